"""Thin torch-tensor front end of the C ABI: validates device/dtype/contiguity, passes raw pointers and
the current HIP stream.  torch is plumbing here (device memory, streams); all arithmetic happens in
libdnmf_hip.so."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib


# bench.py sets TIMING = {} to collect (start, end) HIP events around the named kernels, on their stream
TIMING = None
# launch form of K3n as (passes, chunks), 0 = the library's choice: passes 1 | 2 launches, chunks 1 .. 64 per frame.  The
# tests set it to run every form on small problems; warp_gram_rhs_lists and the *_slots consumers of its tables read it.
LISTS_FORM = (0, 0)
# True: K8's axis transforms run in the vector-ALU kernel kept as the checker of the MFMA one
K8_VALU = False


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if TIMING is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if TIMING is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            TIMING.setdefault(self.name, []).append((self.a, b))


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous float32 CUDA tensor, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")
    return t


def _i32(t, device) -> torch.Tensor:
    if isinstance(t, torch.Tensor):
        return t.to(device=device, dtype=torch.int32).contiguous()
    return torch.tensor(list(t), dtype=torch.int32, device=device)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _rows(t, fn, name, min_row=0, clause=""):
    """``t`` as the kernels take rows: float32 CUDA with unit inner stride (any row stride), at least ``min_row`` floats a
    row (``clause`` says so in the message)."""
    if t.dtype != torch.float32 or t.stride(-1) != 1 or not t.is_cuda or t.shape[-1] < min_row:
        raise ValueError(f"{fn}: {name} must be float32 CUDA with unit inner stride{clause}")
    return t


def _ids(frames, frame_ids, times, dev):
    """``(frame_ids, times, B)``: the two index lists as int32 tensors on ``dev`` (None stays None) and the frames of the
    call -- as many as ``times``, else as ``frame_ids``, else every row of ``frames``."""
    fid = _i32(frame_ids, dev) if frame_ids is not None else None
    tt = _i32(times, dev) if times is not None else None
    return fid, tt, tt.numel() if tt is not None else (fid.numel() if fid is not None else frames.shape[0])


def _nbytes(ws):
    return 0 if ws is None else ws.numel() * ws.element_size()


def _workspace(workspace, need, dev):
    """``workspace`` while it holds ``need`` bytes, else a new float32 one that does."""
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=dev)
    return workspace


def _refused(lib, what):
    return _lib.DnmfHipError(f"{what} refused: {lib.dnmf_last_error().decode(errors='replace')}")


def _need(lib, entry, *args):
    """The bytes the workspace entry ``entry`` asks for; 0 is the library's refusal, raised with its text."""
    need = getattr(lib, entry)(*args)
    if need == 0:
        raise _refused(lib, entry)
    return need


def _stream_state(fn, state, need, first, dev, sized=True):
    """The state of one call of a movie that goes in several: with ``first`` ``state`` while it holds ``need`` bytes, else a new
    one; a later call must bring the state of the earlier ones, with ``sized`` one of ``need`` bytes (without it the library
    judges the size)."""
    if first:
        return _workspace(state, need, dev)
    if state is None or (sized and _nbytes(state) < need):
        size = f", and one of at least {need} bytes (a later call may not be larger than the first)" if sized else ""
        raise ValueError(f"{fn}: first=False needs the state of the earlier calls{size}")
    return state


def _ld(t, P):
    """The row stride of rows ``t``; that of a single row means nothing (a view through numpy's newaxis has 0)."""
    return t.stride(0) if t.shape[0] != 1 else max(t.stride(0), P)


def _frame_rows(fn, frames, sub, frame_ids, P):
    """The checks of every call that reads frames as rows of ``P`` floats -> (frame_ids int32 or None, frames of the call)."""
    _rows(frames, fn, "frames", P, f" and rows of {P} floats")
    if frames.dim() != 2:
        raise ValueError(f"{fn}: frames are rows (T, ld), got {tuple(frames.shape)}")
    fid = _i32(frame_ids, frames.device) if frame_ids is not None else None
    B = fid.numel() if fid is not None else frames.shape[0]
    if sub is not None:
        _rows(sub, fn, "sub", P, f" and rows of {P} floats")
        if sub.dim() != 2 or sub.shape[0] < B:
            raise ValueError(f"{fn}: sub must hold one row for each of the {B} frames, got {tuple(sub.shape)}")
    return fid, B


def _out_rows(fn, out, B, P, dev):
    """``out`` as ``B`` rows of ``P`` floats to write (None: new ones)."""
    if out is None:
        return torch.empty((B, P), dtype=torch.float32, device=dev)
    _rows(out, fn, "out", P, f" and rows of {P} floats")
    if out.dim() != 2 or out.shape[0] < B:
        raise ValueError(f"{fn}: out must hold {B} rows, got {tuple(out.shape)}")
    return out


def _int3(v):
    return (ctypes.c_int * 3)(*[int(x) for x in v])


def build_stamp() -> dict:
    """{source file: hash} the loaded library was compiled from (``dnmf_build_stamp``; dnmf_amd/build.py makes it)."""
    text = _lib.load().dnmf_build_stamp().decode()
    return dict(item.split(":", 1) for item in text.split(";") if ":" in item)


def padded_k(K: int) -> int:
    return _lib.load().dnmf_padded_k(int(K))


HALO = 2   # DNMF_HALO of include/dnmf_hip.h


def halo_voxels(sz) -> int:
    """Floats of one halo-layout image (reconstruction image S, neuron-major footprint At) of the volume ``sz``."""
    X, Y, Z = (int(s) for s in sz)
    return _lib.load().dnmf_halo_voxels(X, Y, Z)


def halo_interior(img: torch.Tensor, sz) -> torch.Tensor:
    """(..., >= halo_voxels) rows in the halo layout -> (..., X, Y, Z) view of the voxels without the border."""
    X, Y, Z = (int(s) for s in sz)
    row = _lib.load().dnmf_halo_row(Y, Z)
    v = img[..., :(X + 2 * HALO) * row].unflatten(-1, (X + 2 * HALO, row))   # views all the way
    return v[..., HALO:HALO + X, HALO * Z:(HALO + Y) * Z].unflatten(-1, (Y, Z))


def pack_footprints(A: torch.Tensor) -> torch.Tensor:
    """A (..., K) -> packed (P, Kp) zero-padded copy the Gram / recon kernels read."""
    K = A.shape[-1]
    A2 = _f32(A.reshape(-1, K), "A")
    Kp = padded_k(K)
    out = torch.empty((A2.shape[0], Kp), dtype=torch.float32, device=A.device)
    _lib.check(_lib.load().dnmf_pack_footprints(A2.data_ptr(), A2.shape[0], K, out.data_ptr(), Kp, _stream()),
               "dnmf_pack_footprints")
    return out


def warp_gather(A: torch.Tensor, beta: torch.Tensor, times, want_A_t=True, want_grid=True):
    """K1.  A (X,Y,Z,K), beta (10,3,T) -> A_t (B,K,X,Y,Z), grid (X,Y,Z,3,B)."""
    X, Y, Z, K = A.shape
    _f32(A, "A"), _f32(beta, "beta")
    tt = _i32(times, A.device)
    B = tt.numel()
    A_t = torch.empty((B, K, X, Y, Z), dtype=torch.float32, device=A.device) if want_A_t else None
    grid = torch.empty((X, Y, Z, 3, B), dtype=torch.float32, device=A.device) if want_grid else None
    _lib.check(_lib.load().dnmf_warp_gather(A.data_ptr(), X, Y, Z, K, beta.data_ptr(), beta.shape[2], tt.data_ptr(), B,
                                            _ptr(A_t), _ptr(grid), _stream()), "dnmf_warp_gather")
    return A_t, grid


def recon_image(Apk: torch.Tensor, K: int, sz, C: torch.Tensor, times, out: torch.Tensor | None = None) -> torch.Tensor:
    """S[b] = sum_k C[k,times[b]] A[:,k] in the halo layout.  Apk (P,Kp), C (K,T) with any row stride (a column window of
    a longer trace table) -> (B, halo_voxels(sz))."""
    X, Y, Z = (int(s) for s in sz)
    _f32(Apk, "Apk"), _rows(C, "recon_image", "C")
    if C.dim() != 2 or C.shape[0] < K:
        raise ValueError(f"recon_image: C must be (K, T) with K = {K} rows, got {tuple(C.shape)}")
    P, Kp = Apk.shape
    if P != X * Y * Z:
        raise ValueError(f"recon_image: Apk has {P} rows, the volume {X}x{Y}x{Z} has {X * Y * Z} voxels")
    tt = _i32(times, Apk.device)
    B = tt.numel()
    lds = halo_voxels(sz)
    if out is None:
        out = torch.empty((B, lds), dtype=torch.float32, device=Apk.device)
    if out.shape[0] < B or out.stride(0) < lds or out.stride(1) != 1:
        raise ValueError("recon_image: out must be (>=B, ld) with ld >= halo_voxels(sz)")
    for s in range(0, B, 32768):   # frames ride on gridDim.y
        n = min(32768, B - s)
        _lib.check(_lib.load().dnmf_recon_image(Apk.data_ptr(), X, Y, Z, K, Kp, C.data_ptr(), C.stride(0),
                                                tt[s:].data_ptr(), n, out[s:].data_ptr(), out.stride(0), _stream()),
                   "dnmf_recon_image")
    return out


def recon_image_lists(layout, K: int, sz, C: torch.Tensor, times, out: torch.Tensor | None = None,
                      skip_empty: bool = False) -> torch.Tensor:
    """S as ``recon_image`` from the K3n layout (``pack_footprints_lists``): compact footprints, static tile lists.  C (K,T)
    with any row stride, as there.  ``skip_empty``: tiles without a neuron are left alone -- only for an ``out`` whose rows
    an earlier call with the same layout and ``skip_empty=False`` has written (they hold zeros there)."""
    X, Y, Z = (int(s) for s in sz)
    _rows(C, "recon_image_lists", "C")
    if C.dim() != 2 or C.shape[0] < K:
        raise ValueError(f"recon_image_lists: C must be (K, T) with K = {K} rows, got {tuple(C.shape)}")
    tt = _i32(times, C.device)
    B = tt.numel()
    lds = halo_voxels(sz)
    if out is None:
        out = torch.empty((B, lds), dtype=torch.float32, device=C.device)
    if out.shape[0] < B or out.stride(0) < lds or out.stride(1) != 1:
        raise ValueError("recon_image_lists: out must be (>=B, ld) with ld >= halo_voxels(sz)")
    with _timed("recon_image_lists"):
        rc = _lib.load().dnmf_recon_image_lists_ex(layout["At"].data_ptr(), layout["bbox"].data_ptr(), K, X, Y, Z,
                                                   C.data_ptr(), C.stride(0), tt.data_ptr(), B, out.data_ptr(),
                                                   out.stride(0), 1 if skip_empty else 0, _stream())
    _lib.check(rc, "dnmf_recon_image_lists_ex")
    return out


def warp_recon_grad(S, s_ids, frames, frame_ids, sz, beta, times, grad=None, gout=None, want_recon=False,
                    want_loss=True, want_reg=True, workspace=None, norm_frames=0):
    """K2.  S (>=B, lds) recon images in the halo layout, frames (>=B, ldf) or None with gout (B,P).
    Returns dict(recon, loss, frame_loss, reg); ``grad`` (10,3,T) is incremented in place."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    dev = beta.device
    _f32(beta, "beta")
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    lib = _lib.load()
    need = lib.dnmf_warp_recon_grad_workspace(X, Y, Z, B)
    workspace = _workspace(workspace, need, dev)
    recon = torch.empty((B, P), dtype=torch.float32, device=dev) if want_recon else None
    loss = torch.empty((1,), dtype=torch.float32, device=dev) if want_loss else None
    frame_loss = torch.empty((B,), dtype=torch.float32, device=dev) if want_loss else None
    reg = torch.empty((B,), dtype=torch.float32, device=dev) if want_reg else None
    sid = _i32(s_ids, dev) if s_ids is not None else None
    if frames is not None:
        _rows(frames, "warp_recon_grad", "frames")
    if gout is not None:
        _f32(gout, "gout")
    with _timed("warp_recon_grad"):
        rc = lib.dnmf_warp_recon_grad(
            S.data_ptr(), S.stride(0), _ptr(sid), _ptr(frames), 0 if frames is None else frames.stride(0), _ptr(fid),
            _ptr(gout), X, Y, Z, beta.data_ptr(), beta.shape[2], tt.data_ptr(), B, int(norm_frames), _ptr(recon),
            _ptr(grad),
            _ptr(loss), _ptr(frame_loss), _ptr(reg), workspace.data_ptr(),
            _nbytes(workspace), _stream())
    _lib.check(rc, "dnmf_warp_recon_grad")
    return {"recon": recon, "loss": loss, "frame_loss": frame_loss, "reg": reg, "workspace": workspace}


def motion_grad_lists(layout, K, sz, C, frames, frame_ids, beta, times, grad, norm_frames, chunk, want=False, workspace=None):
    """The motion gradient of the frames ``times`` from the K3n layout: list reconstruction and K2 alternate over pieces
    of ``chunk`` frames whose images share one buffer (they stay in the Infinity Cache).  ``grad`` (10,3,T) is
    incremented.  Returns dict(frame_loss, reg, workspace) (the first two None unless ``want``)."""
    X, Y, Z = (int(s) for s in sz)
    dev = beta.device
    _f32(beta, "beta"), _f32(C, "C"), _f32(grad, "grad")
    _rows(frames, "motion_grad_lists", "frames")
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    lib = _lib.load()
    chunk = max(1, min(int(chunk), B))
    need = lib.dnmf_motion_grad_lists_workspace(X, Y, Z, chunk, B)
    workspace = _workspace(workspace, need, dev)
    frame_loss = torch.empty((B,), dtype=torch.float32, device=dev) if want else None
    reg = torch.empty((B,), dtype=torch.float32, device=dev) if want else None
    with _timed("motion_grad_lists"):
        rc = lib.dnmf_motion_grad_lists(layout["At"].data_ptr(), layout["bbox"].data_ptr(), K, C.data_ptr(), C.stride(0),
                                        frames.data_ptr(), frames.stride(0), _ptr(fid), X, Y, Z, beta.data_ptr(),
                                        beta.shape[2], tt.data_ptr(), B, int(norm_frames), grad.data_ptr(), _ptr(frame_loss),
                                        _ptr(reg), chunk, workspace.data_ptr(), _nbytes(workspace),
                                        _stream())
    _lib.check(rc, "dnmf_motion_grad_lists")
    return {"frame_loss": frame_loss, "reg": reg, "workspace": workspace}


def warp_normal_eqs(S, s_ids, frames, frame_ids, sz, beta, times, out=None, accumulate=False, workspace=None):
    """K16.  The per-frame normal equations of the motion fit at ``beta[:, :, times]`` in the centred quadratic basis
    (``include/dnmf_hip.h``): ``S`` / ``s_ids`` / ``frames`` / ``frame_ids`` as ``warp_recon_grad`` takes them.  Returns
    dict(H (B,30,30), g (B,30), sse (B), workspace), float64, parameter index a*3+d; ``out``: an earlier result to write into,
    ``accumulate``: add to it instead (colour channels)."""
    X, Y, Z = (int(s) for s in sz)
    dev = beta.device
    _f32(beta, "beta")
    _rows(frames, "warp_normal_eqs", "frames")
    _rows(S, "warp_normal_eqs", "S")
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    if tt is None:
        raise ValueError("warp_normal_eqs: times is required")
    if accumulate and out is None:
        raise ValueError("warp_normal_eqs: accumulate=True needs the earlier result as out")
    lib = _lib.load()
    workspace = _workspace(workspace, lib.dnmf_warp_normal_eqs_workspace(X, Y, Z, B), dev)
    if out is None:
        out = {"H": torch.empty((B, 30, 30), dtype=torch.float64, device=dev),
               "g": torch.empty((B, 30), dtype=torch.float64, device=dev),
               "sse": torch.empty((B,), dtype=torch.float64, device=dev)}
    H, g, sse = out["H"], out["g"], out["sse"]
    for t, shape in ((H, (30, 30)), (g, (30,)), (sse, ())):
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.shape[0] < B or tuple(t.shape[1:]) != shape:
            raise ValueError("warp_normal_eqs: out must hold contiguous float64 CUDA H (>=B,30,30), g (>=B,30), sse (>=B)")
    sid = _i32(s_ids, dev) if s_ids is not None else None
    with _timed("warp_normal_eqs"):
        rc = lib.dnmf_warp_normal_eqs(S.data_ptr(), S.stride(0), _ptr(sid), frames.data_ptr(), frames.stride(0), _ptr(fid),
                                      X, Y, Z, beta.data_ptr(), beta.shape[2], tt.data_ptr(), B, H.data_ptr(), g.data_ptr(),
                                      sse.data_ptr(), 1 if accumulate else 0, workspace.data_ptr(), _nbytes(workspace),
                                      _stream())
    _lib.check(rc, "dnmf_warp_normal_eqs")
    return {"H": H, "g": g, "sse": sse, "workspace": workspace}


def centred_basis_matrix(sz):
    """M (10,10) float64 numpy with ``basis(u(v)) . gamma == basis(v) . (M gamma)`` for every voxel v, where
    ``u_d = 2 x_d / (S_d - 1) - 1`` (0 on an axis of one voxel) and ``basis`` is the reference's
    [1, x, y, z, x^2, y^2, z^2, xy, xz, yz]: coefficients of the centred basis (K16's unknowns) -> coefficients ``beta``."""
    import numpy as np
    s = [2.0 / (int(n) - 1) if int(n) > 1 else 0.0 for n in sz]
    o = [-1.0 if int(n) > 1 else 0.0 for n in sz]
    M = np.zeros((10, 10), dtype=np.float64)
    M[0, 0] = 1.0
    for d in range(3):                       # u_d and u_d^2
        M[0, 1 + d], M[1 + d, 1 + d] = o[d], s[d]
        M[0, 4 + d], M[1 + d, 4 + d], M[4 + d, 4 + d] = o[d] * o[d], 2.0 * s[d] * o[d], s[d] * s[d]
    for c, (p, q) in ((7, (0, 1)), (8, (0, 2)), (9, (1, 2))):   # u_p u_q
        M[0, c], M[1 + p, c], M[1 + q, c], M[c, c] = o[p] * o[q], s[p] * o[q], o[p] * s[q], s[p] * s[q]
    return M


def centred_basis_inverse(sz):
    """Minv (10,10) float64 numpy: the inverse of ``centred_basis_matrix(sz)`` on the active monomials (all 10; the 6 without z
    at Z = 1, where M itself is singular), zeros elsewhere: coefficients ``beta`` -> coefficients of the centred basis."""
    import numpy as np
    M = centred_basis_matrix(sz)
    rows = [a for a in range(10) if int(sz[2]) > 1 or a not in (3, 6, 8, 9)]
    Minv = np.zeros((10, 10), dtype=np.float64)
    Minv[np.ix_(rows, rows)] = np.linalg.inv(M[np.ix_(rows, rows)])
    return Minv


def lm_state(B: int, dev):
    """The per-frame state ``lm_step`` keeps for ``B`` frames (``include/dnmf_hip.h``); only ``counts`` needs its zeros."""
    f64 = dict(dtype=torch.float64, device=dev)
    return {"H": torch.empty((B, 30, 30), **f64), "g": torch.empty((B, 30), **f64), "sse": torch.empty((B,), **f64),
            "sse0": torch.empty((B,), **f64), "lam": torch.empty((B,), **f64),
            "beta": torch.empty((B, 30), dtype=torch.float32, device=dev),
            "counts": torch.zeros((B, 3), dtype=torch.int32, device=dev)}


_CENTRED_M = {}


def _centred(sz, dev):
    """(M, Minv) of the volume on ``dev``, made once."""
    key = (tuple(int(s) for s in sz), str(dev))
    if key not in _CENTRED_M:
        _CENTRED_M[key] = (torch.from_numpy(centred_basis_matrix(sz)).to(dev), torch.from_numpy(centred_basis_inverse(sz)).to(dev))
    return _CENTRED_M[key]


def warp_jacobian_points(sz):
    """(NP,3) float64 numpy: the sample points of the volume-preserving prior (K16j, ``lm_step(jacobian=...)``) in centred
    coordinates, in the kernel's order -- the corners u in {-1, +1}^n counted with the first axis slowest, then the centre u = 0.
    NP = 9; 5 at Z = 1, where u_2 = 0 throughout."""
    import itertools
    import numpy as np
    n = 3 if int(sz[2]) > 1 else 2
    return np.array([list(c) + [0.0] * (3 - n) for c in itertools.product((-1.0, 1.0), repeat=n)] + [[0.0, 0.0, 0.0]])


def lm_step(state, eqs, sz, beta, times, nu=10.0, lam0=1e-3, lam_min=1e-9, lam_max=1e9, accept_only=False, smooth=0.0,
            n_residuals=None, beta_ref=None, jacobian=0.0, order="quadratic"):
    """One Levenberg-Marquardt step per frame on the device (``dnmf_lm_step``).  ``eqs``: ``warp_normal_eqs``' result at the
    trial coefficients ``beta[:, :, times]``; ``state``: ``lm_state(B, device)``.  The trial is accepted when its sse is finite
    and below the accepted one (always on a frame's first call), ``beta[:, :, times]`` then receives the next trial -- or, with
    ``accept_only``, the best accepted coefficients.  Returns ``state``.

    ``smooth`` != 0: the step with the temporal prior (``dnmf_lm_step_smooth``), weight m = ``smooth`` * ``n_residuals`` (default:
    the voxels of ``sz``; pass voxels x colour channels).  ``beta_ref`` (10,3,T) fp32 holds every frame's accepted coefficients:
    read at t +- 1, written at t on accept, never ``beta`` itself.  ``state`` gains ``prior`` (B) float64.  The frames of one call
    must be pairwise non-adjacent; a ``times`` given as a host sequence is checked, a device tensor is the caller's word.

    ``order`` (``WARP_ORDERS``): ``'translation'`` or ``'affine'`` step on the rows of the centred basis of that degree only
    (K16o, ``dnmf_lm_step_order``; with or without the prior) and leave the other rows of ``beta[:, :, times]`` as they are, bit
    for bit; ``eqs`` is the same.  ``'quadratic'``, the default, is the two entries above.

    ``jacobian`` != 0: the step with the volume-preserving prior (K16j, ``dnmf_lm_step_jac``, whatever ``order`` and ``smooth``
    are), weight m_j = ``jacobian`` * ``n_residuals``: J = m_j mean_p (log det Jx(u_p))^2 over ``warp_jacobian_points(sz)``, Jx the
    Jacobian of the frame's map in voxel coordinates, +inf for a map that folds at a sample point -- so a folded trial is never
    accepted after a frame's first call.  ``state`` gains ``jac`` (B) float64, J of the point kept, and ``min_det`` (B), its
    smallest det Jx over the sample points.  0.0, the default, takes the entries above."""
    if order not in WARP_ORDERS:
        raise ValueError(f"lm_step: order must be one of {sorted(WARP_ORDERS)}, got {order!r}")
    jacobian = float(jacobian)
    if not (jacobian >= 0.0 and jacobian != float("inf")):
        raise ValueError(f"lm_step: jacobian={jacobian}: expected a finite weight >= 0")
    dev = beta.device
    _f32(beta, "beta")
    smooth = float(smooth)
    if smooth != 0.0:
        if not (smooth > 0.0 and smooth != float("inf")):
            raise ValueError(f"lm_step: smooth={smooth}: expected a finite weight >= 0")
        if not isinstance(times, torch.Tensor):
            host = sorted(int(t) for t in times)
            if any(b - a == 1 for a, b in zip(host, host[1:])):
                raise ValueError("lm_step: smooth != 0 needs pairwise non-adjacent frames in one call (one parity of t at a "
                                 f"time), got times={list(times)}")
        if beta_ref is None or beta_ref.shape != beta.shape or beta_ref.data_ptr() == beta.data_ptr():
            raise ValueError("lm_step: smooth != 0 needs beta_ref, a float32 CUDA tensor shaped like beta and not beta itself")
        _f32(beta_ref, "beta_ref")
    tt = _i32(times, dev)
    B = tt.numel()
    H, g, sse = eqs["H"], eqs["g"], eqs["sse"]
    if min(H.shape[0], g.shape[0], sse.shape[0], *(state[k].shape[0] for k in ("H", "g", "sse", "sse0", "lam", "beta", "counts"))) < B:
        raise ValueError(f"lm_step: {B} frames, but the normal equations or the state hold fewer")
    for name, t in (("H", H), ("g", g), ("sse", sse)):
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"lm_step: {name} must be a contiguous float64 CUDA tensor")
    M, Minv = _centred(sz, dev)
    if smooth != 0.0 and ("prior" not in state or state["prior"].shape[0] < B):
        state["prior"] = torch.zeros((state["counts"].shape[0],), dtype=torch.float64, device=dev)
    n = int(sz[0]) * int(sz[1]) * int(sz[2]) if n_residuals is None else int(n_residuals)
    if jacobian != 0.0:
        for key in ("jac", "min_det"):
            if key not in state or state[key].shape[0] < B:
                state[key] = torch.zeros((state["counts"].shape[0],), dtype=torch.float64, device=dev)
        rc = _lib.load().dnmf_lm_step_jac(H.data_ptr(), g.data_ptr(), sse.data_ptr(), B, int(sz[0]), int(sz[1]), int(sz[2]),
                                          WARP_ORDERS[order], M.data_ptr(), Minv.data_ptr(), beta.data_ptr(), beta.shape[2],
                                          tt.data_ptr(), state["H"].data_ptr(), state["g"].data_ptr(), state["sse"].data_ptr(),
                                          state["sse0"].data_ptr(), state["lam"].data_ptr(), state["beta"].data_ptr(),
                                          state["counts"].data_ptr(), float(nu), float(lam0), float(lam_min), float(lam_max),
                                          1 if accept_only else 0, beta_ref.data_ptr() if smooth else None, smooth * n,
                                          state["prior"].data_ptr() if smooth else None, jacobian * n, state["jac"].data_ptr(),
                                          state["min_det"].data_ptr(), _stream())
        _lib.check(rc, "dnmf_lm_step_jac")
        return state
    if order != "quadratic":
        rc = _lib.load().dnmf_lm_step_order(H.data_ptr(), g.data_ptr(), sse.data_ptr(), B, int(sz[2]), WARP_ORDERS[order], M.data_ptr(),
                                            Minv.data_ptr(), beta.data_ptr(), beta.shape[2], tt.data_ptr(), state["H"].data_ptr(),
                                            state["g"].data_ptr(), state["sse"].data_ptr(), state["sse0"].data_ptr(),
                                            state["lam"].data_ptr(), state["beta"].data_ptr(), state["counts"].data_ptr(), float(nu),
                                            float(lam0), float(lam_min), float(lam_max), 1 if accept_only else 0,
                                            beta_ref.data_ptr() if smooth else None, smooth * n,
                                            state["prior"].data_ptr() if smooth else None, _stream())
        _lib.check(rc, "dnmf_lm_step_order")
        return state
    if smooth == 0.0:
        rc = _lib.load().dnmf_lm_step(H.data_ptr(), g.data_ptr(), sse.data_ptr(), B, int(sz[2]), M.data_ptr(), beta.data_ptr(),
                                      beta.shape[2], tt.data_ptr(), state["H"].data_ptr(), state["g"].data_ptr(),
                                      state["sse"].data_ptr(), state["sse0"].data_ptr(), state["lam"].data_ptr(),
                                      state["beta"].data_ptr(), state["counts"].data_ptr(), float(nu), float(lam0), float(lam_min),
                                      float(lam_max), 1 if accept_only else 0, _stream())
        _lib.check(rc, "dnmf_lm_step")
        return state
    rc = _lib.load().dnmf_lm_step_smooth(H.data_ptr(), g.data_ptr(), sse.data_ptr(), B, int(sz[2]), M.data_ptr(), Minv.data_ptr(),
                                         beta.data_ptr(), beta.shape[2], tt.data_ptr(), state["H"].data_ptr(),
                                         state["g"].data_ptr(), state["sse"].data_ptr(), state["sse0"].data_ptr(),
                                         state["lam"].data_ptr(), state["beta"].data_ptr(), state["counts"].data_ptr(), float(nu),
                                         float(lam0), float(lam_min), float(lam_max), 1 if accept_only else 0, beta_ref.data_ptr(),
                                         smooth * n, state["prior"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_lm_step_smooth")
    return state


def _gram_out(out, B, K, dev, fn):
    """``(G, r)``: new (B,K,K) and (B,K) tensors, or the caller's pair ``out`` after a check of what the kernels write."""
    if out is None:
        return torch.empty((B, K, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.float32, device=dev)
    G, r = out
    _f32(G, "out[0]"), _f32(r, "out[1]")
    if tuple(G.shape) != (B, K, K) or tuple(r.shape) != (B, K):
        raise ValueError(f"{fn}: out must be (G ({B},{K},{K}), r ({B},{K})), got {tuple(G.shape)} and {tuple(r.shape)}")
    return G, r


def warp_gram_rhs(Apk, K, sz, beta, times, frames, frame_ids=None, a_frame_stride=0, workspace=None, bf16=False, out=None):
    """K3 (``bf16=True``: K3b, operands rounded to bf16, fp32 accumulate).  Returns G (B,K,K), r (B,K) for the
    frames listed (written into the pair ``out`` when given).  ``beta`` None: no warp (each voxel's own footprint row,
    weight 1)."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    dev = Apk.device
    _f32(Apk, "Apk")
    if beta is not None:
        _f32(beta, "beta")
    lib = _lib.load()
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    _rows(frames, "warp_gram_rhs", "frames")
    need = lib.dnmf_warp_gram_rhs_workspace(P, K, B)
    workspace = _workspace(workspace, need, dev)
    G, r = _gram_out(out, B, K, dev, "warp_gram_rhs")
    with _timed("warp_gram_rhs_bf16" if bf16 else "warp_gram_rhs"):
        rc = (lib.dnmf_warp_gram_rhs_bf16 if bf16 else lib.dnmf_warp_gram_rhs)(
            Apk.data_ptr(), Apk.shape[-1], K, a_frame_stride, X, Y, Z, _ptr(beta), B if beta is None else beta.shape[2],
            _ptr(tt), B, frames.data_ptr(), frames.stride(0), _ptr(fid), G.data_ptr(), r.data_ptr(), workspace.data_ptr(),
            _nbytes(workspace), _stream())
    _lib.check(rc, "dnmf_warp_gram_rhs")
    return G, r, workspace


def _state(fn, C, dtype, name="C", shape=""):
    """The (K,T) state of a trace update (K4, K4h, K32) as the kernels take it: ``dtype`` CUDA, unit inner stride, any row stride."""
    if not (C.is_cuda and C.dtype == dtype and C.dim() == 2 and C.stride(1) == 1):
        raise ValueError(f"{fn}: {name} must be {str(dtype).split('.')[-1]} CUDA{shape} with unit inner stride")


def mu_temporal(G, r, C, iters: int, nbr=None):
    """K4 without the neighbour term: C (K,T) fp32 updated in place.  ``nbr`` (K,NN) int32: the columns of G that
    can be non-zero per row (``pack_footprints_lists``) -- same result while every trace is finite, NN instead of K terms
    per row."""
    _f32(G, "G"), _f32(r, "r")
    _state("mu_temporal", C, torch.float32)
    T, K = r.shape
    if nbr is not None:
        _lib.check(_lib.load().dnmf_mu_temporal_nbr(G.data_ptr(), r.data_ptr(), C.data_ptr(), C.stride(0), K, T, int(iters),
                                                    nbr.data_ptr(), nbr.shape[1], _stream()), "dnmf_mu_temporal_nbr")
        return C
    _lib.check(_lib.load().dnmf_mu_temporal(G.data_ptr(), r.data_ptr(), C.data_ptr(), C.stride(0), K, T, int(iters),
                                            _stream()), "dnmf_mu_temporal")
    return C


def mu_temporal_step(G, r, Cin, Cout, gamma: float, c_left=None, c_right=None):
    """K4, one round with the neighbour term; Cin/Cout (K,T) float64 with the same row stride (the ABI has one ldc)."""
    _f32(G, "G"), _f32(r, "r")
    _state("mu_temporal_step", Cin, torch.float64, "Cin"), _state("mu_temporal_step", Cout, torch.float64, "Cout")
    if Cout.stride(0) != Cin.stride(0):
        raise ValueError(f"mu_temporal_step: Cin and Cout must have the same row stride, got Cin.stride(0)="
                         f"{Cin.stride(0)} and Cout.stride(0)={Cout.stride(0)}")
    T, K = r.shape
    _lib.check(_lib.load().dnmf_mu_temporal_step(G.data_ptr(), r.data_ptr(), Cin.data_ptr(), Cout.data_ptr(),
                                                 Cin.stride(0), K, T, float(gamma), _ptr(c_left), _ptr(c_right),
                                                 _stream()), "dnmf_mu_temporal_step")
    return Cout


def _nbr_table(fn, nbr, K):
    """``(pointer, NN)`` of an optional (K,NN) int32 neighbour table."""
    if nbr is None:
        return 0, 0
    if not (nbr.is_cuda and nbr.dtype == torch.int32 and nbr.is_contiguous() and nbr.dim() == 2 and nbr.shape[0] == K):
        raise ValueError(f"{fn}: nbr must be a contiguous int32 CUDA tensor of shape (K={K}, NN)")
    return nbr.data_ptr(), nbr.shape[1]


def _gram_against_state(fn, G, r, C):
    """Shapes of G (T,K,K), r (T,K) against the state C (K,T); returns (K, T)."""
    _f32(G, "G"), _f32(r, "r")
    K, T = C.shape
    if tuple(r.shape) != (T, K) or tuple(G.shape) != (T, K, K):
        raise ValueError(f"{fn}: G {tuple(G.shape)}, r {tuple(r.shape)} do not match C (K={K}, T={T})")
    return K, T


def hals_temporal(G, r, C, iters: int, nbr=None, kkt=False):
    """K4h without the neighbour term: ``iters`` sweeps of cyclic coordinate descent (k ascending) on
    ``1/2 c^T G_t c - r_t^T c, c >= 0`` per frame; C (K,T) fp32 updated in place.  ``nbr`` as for ``mu_temporal``.
    ``kkt=True``: returns ``(C, kkt)``, kkt (T) float64 = the largest projected-gradient entry per frame after the last
    sweep (zero at the NNLS solution)."""
    _state("hals_temporal", C, torch.float32)
    K, T = _gram_against_state("hals_temporal", G, r, C)
    if int(iters) < 0:
        raise ValueError(f"hals_temporal: iters={iters} < 0")
    pn, NN = _nbr_table("hals_temporal", nbr, K)
    out = torch.empty((T,), dtype=torch.float64, device=C.device) if kkt else None
    with _timed("hals_temporal"):
        rc = _lib.load().dnmf_hals_temporal(G.data_ptr(), r.data_ptr(), C.data_ptr(), C.stride(0), K, T, int(iters), pn, NN,
                                            _ptr(out), _stream())
    _lib.check(rc, "dnmf_hals_temporal")
    return (C, out) if kkt else C


def hals_temporal_step(G, r, C, gamma: float, parity: int, nbr=None):
    """K4h, one half sweep with the neighbour term on the fp64 state C (K,T), in place: the frames ``parity, parity + 2,
    ...`` are updated.  A sweep is parity 0, then parity 1."""
    _state("hals_temporal_step", C, torch.float64)
    if parity not in (0, 1):
        raise ValueError(f"hals_temporal_step: parity={parity!r}, expected 0 or 1")
    K, T = _gram_against_state("hals_temporal_step", G, r, C)
    pn, NN = _nbr_table("hals_temporal_step", nbr, K)
    with _timed("hals_temporal_step"):
        rc = _lib.load().dnmf_hals_temporal_step(G.data_ptr(), r.data_ptr(), C.data_ptr(), C.stride(0), K, T, float(gamma),
                                                 int(parity), pn, NN, _stream())
    _lib.check(rc, "dnmf_hals_temporal_step")
    return C


def hals_temporal_kkt(G, r, C, gamma: float = 0.0, nbr=None):
    """(T) float64: the largest projected-gradient entry per frame of the fp64 state C (K,T) under ``gamma`` (the measure
    ``hals_temporal(..., kkt=True)`` returns, for any state and with the neighbour term)."""
    _state("hals_temporal_kkt", C, torch.float64)
    K, T = _gram_against_state("hals_temporal_kkt", G, r, C)
    pn, NN = _nbr_table("hals_temporal_kkt", nbr, K)
    out = torch.empty((T,), dtype=torch.float64, device=C.device)
    with _timed("hals_temporal_kkt"):
        rc = _lib.load().dnmf_hals_temporal_kkt(G.data_ptr(), r.data_ptr(), C.data_ptr(), C.stride(0), K, T,
                                                0.0 if gamma is None else float(gamma), pn, NN, out.data_ptr(), _stream())
    _lib.check(rc, "dnmf_hals_temporal_kkt")
    return out


def render_frames(positions, traces, sz, shape_std, t0=0, T=None, out=None):
    """Simulator render loop on the GPU: frames t0..t0+T-1 of the video as (T,P) fp32."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    pos = _f32(positions, "positions")
    if not (traces.is_cuda and traces.dtype == torch.float64 and traces.is_contiguous()):
        raise ValueError("render_frames: traces must be a contiguous float64 CUDA tensor")
    K, _, T_total = pos.shape
    T = T_total - t0 if T is None else int(T)
    if out is None:
        out = torch.empty((T, P), dtype=torch.float32, device=pos.device)
    lib = _lib.load()
    amp = float(traces.abs().max())   # the kernel's cut-off is sized for the largest magnitude: a negative trace counts
    for s in range(0, T, 32768):
        n = min(32768, T - s)
        _lib.check(lib.dnmf_render_frames(pos.data_ptr(), traces.data_ptr(), K, T_total, t0 + s, n, X, Y, Z,
                                          float(shape_std), amp, out[s:].data_ptr(), out.stride(0), _stream()),
                   "dnmf_render_frames")
    return out


def adam_epoch(beta, grad, exp_avg, exp_avg_sq, step0, frame_step, nsteps, lr, betas, eps, phase, order=None):
    """One phase of the per-column Adam epoch (see include/dnmf_hip.h); tensors updated in place.  ``order`` (T)
    int32: the frames sorted by ``frame_step`` (speed only)."""
    for t, n in ((beta, "beta"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _f32(t, n)
    if grad is not None:
        _f32(grad, "grad")
    fs = _i32(frame_step, beta.device)
    od = _i32(order, beta.device) if order is not None else None
    ws = torch.empty((4 * int(nsteps),), dtype=torch.float32, device=beta.device)
    _lib.check(_lib.load().dnmf_adam_epoch(beta.data_ptr(), _ptr(grad), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                           beta.shape[2], int(step0), fs.data_ptr(), _ptr(od), int(nsteps), float(lr),
                                           float(betas[0]), float(betas[1]), float(eps), int(phase), ws.data_ptr(),
                                           ws.numel() * 4, _stream()),
               "dnmf_adam_epoch")


def spatial_accum(Y, C, frame_ids=None, times=None, A1=None, Cs=None, accumulate=False):
    """K5.  Y (>=T, ldy) frames, C (K, ldc) traces -> A1 (P,K) = Y^T C^T over the frames, Cs (K,K) = C C^T."""
    _rows(Y, "spatial_accum", "Y"), _rows(C, "spatial_accum", "C")
    dev = Y.device
    fid, tt, T = _ids(Y, frame_ids, times, dev)
    P, K = Y.shape[1], C.shape[0]
    if A1 is None:
        A1 = torch.empty((P, K), dtype=torch.float32, device=dev)
        Cs = torch.empty((K, K), dtype=torch.float32, device=dev)
        accumulate = False
    Ct = C.t().contiguous()   # frame-major copy of the traces (K T floats): the kernel's matrix operands in 64-byte runs
    # (the transpose of a single trace column is contiguous as it stands and keeps stride 1: _ld, as for any single row)
    with _timed("spatial_accum"):
        rc = _lib.load().dnmf_spatial_accum(Y.data_ptr(), _ld(Y, P), _ptr(fid), C.data_ptr(), _ld(C, C.shape[1]), Ct.data_ptr(),
                                            _ld(Ct, K), _ptr(tt), T, P, K, A1.data_ptr(), Cs.data_ptr(),
                                            int(bool(accumulate)), _stream())
    _lib.check(rc, "dnmf_spatial_accum")
    return A1, Cs


def mu_spatial(A, A1, Cs, D=None, gamma=0.0):
    """K6.  A (P,K) fp32 updated in place: A * A1 / (A Cs + gamma D + 1e-32)."""
    for t, n in ((A, "A"), (A1, "A1"), (Cs, "Cs")):
        _f32(t, n)
    if D is not None:
        _f32(D, "D")
    P, K = A.shape
    with _timed("mu_spatial"):
        rc = _lib.load().dnmf_mu_spatial(A.data_ptr(), A1.data_ptr(), Cs.data_ptr(), _ptr(D), float(gamma or 0.0), P, K,
                                         _stream())
    _lib.check(rc, "dnmf_mu_spatial")
    return A


def spatial_lists_setup(layout, K, sz):
    """Tile lists of the list-form footprint update from the boxes of ``pack_footprints_lists``: dict(tables int32,
    total) -- ``total`` floats of the compact A1 buffer, or -1 when a tile lists more than 32 neurons (use the dense K5)."""
    X, Y, Z = (int(s) for s in sz)
    lib = _lib.load()
    nt = lib.dnmf_spatial_lists_tiles(X, Y, Z)
    tables = torch.empty((2 * nt + 2 + 32 * nt,), dtype=torch.int32, device=layout["bbox"].device)
    _lib.check(lib.dnmf_spatial_lists_setup(layout["bbox"].data_ptr(), K, X, Y, Z, tables.data_ptr(), _stream()),
               "dnmf_spatial_lists_setup")
    return {"tables": tables, "total": int(tables[2 * nt].item()), "ntiles": nt}


def spatial_accum_lists(Y, C, sl, sz, K, frame_ids=None, times=None, A1c=None, Cs=None, workspace=None):
    """K5, list form.  Y (>=T, ldy) registered frames, C (K, ldc) -> A1c (total) compact sums, Cs (K,K)."""
    return _spatial_accum_lists("spatial_accum_lists", Y, C, None, sl, sz, K, frame_ids, times, A1c, Cs, workspace)


def spatial_accum_lists_channels(Y, C, colours, sl, sz, K, frame_ids=None, times=None, A1c=None, Cs=None, workspace=None):
    """K5, list form over colour channels: Y (>=T, ldy) rows of NC channels of P floats, colours (NC,K) ->
    A1c (total) = sum_c colours[c,k] (Y^c C^T) at the listed entries, Cs (K,K) = C C^T."""
    return _spatial_accum_lists("spatial_accum_lists_channels", Y, C, colours, sl, sz, K, frame_ids, times, A1c, Cs, workspace)


def _spatial_accum_lists(fn, Y, C, colours, sl, sz, K, frame_ids, times, A1c, Cs, workspace):
    """The list-form K5 behind both entry points: ``colours`` None is the single-channel kernel ``dnmf_spatial_accum_lists``."""
    X, Yd, Z = (int(s) for s in sz)
    P = X * Yd * Z
    if colours is None:
        _rows(Y, fn, "Y")
    else:
        _f32(colours, "colours")
        NC = colours.shape[0]
        if colours.dim() != 2 or colours.shape[1] != K:
            raise ValueError(f"{fn}: colours must be (NC, K={K}), got {tuple(colours.shape)}")
        _rows(Y, fn, "Y", NC * P, f" and rows of {NC} x {P}")
    _rows(C, fn, "C")
    dev = Y.device
    fid, tt, T = _ids(Y, frame_ids, times, dev)
    total = sl["total"]
    if A1c is None:
        A1c = torch.empty((total,), dtype=torch.float32, device=dev)
        Cs = torch.empty((K, K), dtype=torch.float32, device=dev)
    lib = _lib.load()
    need = lib.dnmf_spatial_accum_lists_workspace(X, Yd, Z, total, T)
    if need:   # 0: these frames go in one pass, no workspace (None is passed on as such)
        workspace = _workspace(workspace, need, dev)
    tail = (_ptr(tt), T, X, Yd, Z, K, sl["tables"].data_ptr(), total, A1c.data_ptr(), Cs.data_ptr(), _ptr(workspace),
            _nbytes(workspace), _stream())
    with _timed("spatial_accum_lists"):
        if colours is None:
            rc = lib.dnmf_spatial_accum_lists(Y.data_ptr(), Y.stride(0), _ptr(fid), C.data_ptr(), C.stride(0), *tail)
        else:
            rc = lib.dnmf_spatial_accum_lists_channels(Y.data_ptr(), Y.stride(0), P, NC, colours.data_ptr(), _ptr(fid),
                                                       C.data_ptr(), C.stride(0), *tail)
    _lib.check(rc, "dnmf_" + fn)
    return A1c, Cs, workspace


def mu_spatial_lists(A, layout, sl, A1c, Cs, sz, D=None, gamma=0.0):
    """K6, list form: A (P,K) updated in place at the entries the tiles list; A1c is overwritten with the new values."""
    X, Y, Z = (int(s) for s in sz)
    for t, n in ((A, "A"), (A1c, "A1c"), (Cs, "Cs")):
        _f32(t, n)
    if D is not None:
        _f32(D, "D")
    with _timed("mu_spatial_lists"):
        rc = _lib.load().dnmf_mu_spatial_lists(A.data_ptr(), layout["At"].data_ptr(), A1c.data_ptr(), Cs.data_ptr(), _ptr(D),
                                               float(gamma or 0.0), X, Y, Z, A.shape[1], sl["tables"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_mu_spatial_lists")
    return A


def _hals_spatial_boxes(fn, boxes, K, sz, dev):
    """``boxes`` (K,6) as an int32 tensor on ``dev`` with ``sz``; a box that is not empty must lie inside the volume."""
    if sz is None:
        raise ValueError(f"{fn}: boxes need the volume sz=(X, Y, Z)")
    sz = tuple(int(s) for s in sz)
    b = torch.as_tensor(boxes)
    if b.is_floating_point() or b.dim() != 2 or tuple(b.shape) != (K, 6):
        raise ValueError(f"{fn}: boxes must be integers of shape (K={K}, 6), got {b.dtype} {tuple(b.shape)}")
    b = b.to(device=dev, dtype=torch.int32).contiguous()
    lo, hi = b[:, 0::2].long(), b[:, 1::2].long()
    full = (lo <= hi).all(1, keepdim=True)
    dims = torch.tensor(sz, device=dev)
    if bool((full & ((lo < 0) | (hi >= dims))).any()):
        raise ValueError(f"{fn}: a box reaches outside the volume {sz}")
    return b, sz


def _hals_spatial_sums(fn, A, A1, Cs, D):
    for t, n in ((A, "A"), (A1, "A1"), (Cs, "Cs")):
        _f32(t, n)
    if A.dim() != 2 or A1.shape != A.shape or tuple(Cs.shape) != (A.shape[1], A.shape[1]):
        raise ValueError(f"{fn}: A {tuple(A.shape)} (P,K), A1 {tuple(A1.shape)} (P,K) and Cs {tuple(Cs.shape)} (K,K) do not match")
    if D is not None and _f32(D, "D").shape != A.shape:
        raise ValueError(f"{fn}: D {tuple(D.shape)} is not like A {tuple(A.shape)}")
    return A.shape


def _sweeps(fn, sweeps):
    if int(sweeps) != sweeps or sweeps < 1:
        raise ValueError(f"{fn}: sweeps={sweeps!r}, a whole number >= 1")
    return int(sweeps)


def hals_spatial(A, A1, Cs, D=None, gamma=0.0, sweeps=1, boxes=None, kkt=False, sz=None):
    """K6h, dense form.  A (P,K) fp32 updated in place by ``sweeps`` sweeps of cyclic coordinate descent (k ascending) on
    ``1/2 a^T Cs a - A1[p]^T a + gamma D[p]^T a, a >= 0`` per voxel, over the neurons whose box holds it: ``boxes`` (K,6)
    integers (xlo, xhi, ylo, yhi, zlo, zhi), inclusive, with the volume ``sz`` -- values outside become 0 -- or None: every
    voxel is free.  ``kkt=True``: returns ``(A, kkt)``, kkt (K) float64 = the largest projected-gradient entry per neuron
    of the float64 state after the last sweep (zero at the NNLS solution)."""
    P, K = _hals_spatial_sums("hals_spatial", A, A1, Cs, D)
    sweeps = _sweeps("hals_spatial", sweeps)
    b, (X, Y, Z) = (None, (0, 0, 0)) if boxes is None else _hals_spatial_boxes("hals_spatial", boxes, K, sz, A.device)
    if b is not None and X * Y * Z != P:
        raise ValueError(f"hals_spatial: sz={sz} does not hold the P={P} voxels of A")
    out = torch.empty((K,), dtype=torch.float64, device=A.device) if kkt else None
    with _timed("hals_spatial"):
        rc = _lib.load().dnmf_hals_spatial(A.data_ptr(), A1.data_ptr(), Cs.data_ptr(), _ptr(D), float(gamma or 0.0), P, K, sweeps,
                                           _ptr(b), X, Y, Z, _ptr(out), _stream())
    _lib.check(rc, "dnmf_hals_spatial")
    return (A, out) if kkt else A


def hals_spatial_kkt(A, A1, Cs, D=None, gamma=0.0, boxes=None, sz=None):
    """(K) float64: the largest projected-gradient entry per neuron of the stored fp32 footprints A (P,K) for the sums
    ``A1``, ``Cs`` (the measure ``hals_spatial(..., kkt=True)`` returns, for any stored state); nothing is written."""
    P, K = _hals_spatial_sums("hals_spatial_kkt", A, A1, Cs, D)
    b, (X, Y, Z) = (None, (0, 0, 0)) if boxes is None else _hals_spatial_boxes("hals_spatial_kkt", boxes, K, sz, A.device)
    if b is not None and X * Y * Z != P:
        raise ValueError(f"hals_spatial_kkt: sz={sz} does not hold the P={P} voxels of A")
    out = torch.empty((K,), dtype=torch.float64, device=A.device)
    with _timed("hals_spatial_kkt"):
        rc = _lib.load().dnmf_hals_spatial_kkt(A.data_ptr(), A1.data_ptr(), Cs.data_ptr(), _ptr(D), float(gamma or 0.0), P, K,
                                               _ptr(b), X, Y, Z, out.data_ptr(), _stream())
    _lib.check(rc, "dnmf_hals_spatial_kkt")
    return out


def hals_spatial_lists(A, layout, sl, A1c, Cs, sz, D=None, gamma=0.0, sweeps=1, kkt=False, bbox=None):
    """K6h, list form, with the arguments of ``mu_spatial_lists``: A (P,K) updated in place at the entries the tiles list
    from the halo copy ``layout["At"]``; A1c in = the sums, out = the new values.  The boxes are ``layout["bbox"]``, or
    ``bbox`` (K,6) where the tile lists ``sl`` were made from other (dilated) boxes.  ``kkt`` as in ``hals_spatial``."""
    X, Y, Z = (int(s) for s in sz)
    for t, n in ((A, "A"), (A1c, "A1c"), (Cs, "Cs")):
        _f32(t, n)
    if A.dim() != 2 or A.shape[0] != X * Y * Z or tuple(Cs.shape) != (A.shape[1], A.shape[1]):
        raise ValueError(f"hals_spatial_lists: A {tuple(A.shape)} (P,K), Cs {tuple(Cs.shape)} (K,K) do not match sz={tuple(sz)}")
    if sl["total"] <= 0 or A1c.numel() < sl["total"]:
        raise ValueError(f"hals_spatial_lists: A1c holds {A1c.numel()} floats, the tile lists {sl['total']} (<= 0: no list form)")
    if D is not None and _f32(D, "D").shape != A.shape:
        raise ValueError(f"hals_spatial_lists: D {tuple(D.shape)} is not like A {tuple(A.shape)}")
    sweeps = _sweeps("hals_spatial_lists", sweeps)
    K = A.shape[1]
    b, _ = _hals_spatial_boxes("hals_spatial_lists", layout["bbox"] if bbox is None else bbox, K, sz, A.device)
    lib = _lib.load()
    out = ws = None
    if kkt:
        out = torch.empty((K,), dtype=torch.float64, device=A.device)
        ws = torch.empty((_need(lib, "dnmf_hals_spatial_lists_workspace", X, Y, Z) // 8,), dtype=torch.float64, device=A.device)
    with _timed("hals_spatial_lists"):
        rc = lib.dnmf_hals_spatial_lists(A.data_ptr(), layout["At"].data_ptr(), A1c.data_ptr(), Cs.data_ptr(), _ptr(D),
                                         float(gamma or 0.0), X, Y, Z, K, sl["tables"].data_ptr(), b.data_ptr(), sweeps, _ptr(out),
                                         _ptr(ws), _nbytes(ws), _stream())
    _lib.check(rc, "dnmf_hals_spatial_lists")
    return (A, out) if kkt else A


def dilate_boxes(bbox, sz, grow):
    """(K,6) int32 boxes grown by ``grow`` voxels -- an int or (gx, gy, gz) -- on every side and clipped to the volume; an
    empty box (lo > hi on an axis) stays as it is."""
    g = [int(v) for v in grow] if hasattr(grow, "__len__") else [int(grow)] * 3
    if len(g) != 3 or min(g) < 0:
        raise ValueError(f"grow={grow!r}: a number of voxels >= 0 or three of them")
    b = bbox.to(torch.int32)
    lo, hi = b[:, 0::2], b[:, 1::2]
    full = (lo <= hi).all(1, keepdim=True)
    gt = torch.tensor(g, dtype=torch.int32, device=b.device)
    top = torch.tensor([int(s) - 1 for s in sz], dtype=torch.int32, device=b.device)
    out = torch.empty_like(b)
    out[:, 0::2] = torch.where(full, (lo - gt).clamp_min(0), lo)
    out[:, 1::2] = torch.where(full, torch.minimum(hi + gt, top), hi)
    return out.contiguous()


def pack_footprints_lists(A, sz):
    """Layout of K3n: dict(At (K,P), bbox (K,6) int32, pair_slot (K,K) int32, nslot int, boxfrac) -- ``boxfrac`` is
    the summed volume of the footprint boxes over the volume, i.e. the mean number of listed neurons per voxel."""
    X, Y, Z = (int(s) for s in sz)
    K = A.shape[-1]
    A2 = _f32(A.reshape(-1, K), "A")
    dev = A.device
    lib = _lib.load()
    At = torch.empty((K, halo_voxels(sz)), dtype=torch.float32, device=dev)   # halo layout, border zeroed by the call
    bbox = torch.empty((K, 6), dtype=torch.int32, device=dev)
    pair_slot = torch.empty((K, K), dtype=torch.int32, device=dev)
    nslot = torch.zeros((1,), dtype=torch.int32, device=dev)
    axis_masks = torch.empty((lib.dnmf_lists_axis_masks_bytes(X, Y, Z, K) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.dnmf_pack_footprints_lists(A2.data_ptr(), X, Y, Z, K, At.data_ptr(), bbox.data_ptr(),
                                              pair_slot.data_ptr(), nslot.data_ptr(), axis_masks.data_ptr(), _stream()),
               "dnmf_pack_footprints_lists")
    bb = bbox.cpu().long()
    ext = (bb[:, 1::2] - bb[:, 0::2] + 1).clamp_min(0)
    ns = int(nslot.item())
    # per row of G the columns inside the pattern, ascending, padded with columns outside it (for K4)
    pattern = pair_slot != ns - 1
    widest = int(pattern.sum(1).max().item())
    NN = next((n for n in (8, 16, 32) if widest <= n <= K), None)
    nbr = None
    if NN is not None:
        nbr = torch.argsort((~pattern).to(torch.uint8), dim=1, stable=True)[:, :NN].to(torch.int32).contiguous()
    return {"At": At, "bbox": bbox, "pair_slot": pair_slot, "nslot": ns, "nbr": nbr, "axis_masks": axis_masks,
            "boxfrac": float(ext.prod(1).sum()) / (X * Y * Z)}


LISTS_MAX_SLOTS = 3800
# executed-work counters of the K3n launches while bench.py's TIMING is on (int64[2] tensor)
LISTS_COUNTERS = None


def _lists_form(passes, chunks):
    """(passes, chunks) of a K3n launch: the arguments, or ``LISTS_FORM`` where they are None."""
    return (int(LISTS_FORM[0] if passes is None else passes), int(LISTS_FORM[1] if chunks is None else chunks))


def _lists_tables(sz, B, passes=None, chunks=None):
    """Slot tables per frame that a K3n launch of B frames in the form (passes, chunks) leaves in its workspace."""
    X, Y, Z = (int(s) for s in sz)
    n = _lib.load().dnmf_warp_gram_rhs_lists_chunks(X, Y, Z, int(B), *_lists_form(passes, chunks))
    if n <= 0:
        raise ValueError(f"K3n: no launch form passes, chunks = {_lists_form(passes, chunks)} on {X}x{Y}x{Z}, {B} frames")
    return n


def warp_gram_rhs_lists(layout, K, sz, beta, times, frames, frame_ids=None, workspace=None, finish=True, out=None,
                        passes=None, chunks=None):
    """K3n.  Returns G (B,K,K), r (B,K), workspace (G and r written into the pair ``out`` when given); with
    ``finish=False`` G and r are None and the slot tables stay in ``workspace`` for ``mu_temporal_slots``.
    ``passes``, ``chunks``: the launch form (None: from ``LISTS_FORM``; 0: the library's choice)."""
    global LISTS_COUNTERS
    X, Y, Z = (int(s) for s in sz)
    dev = beta.device
    _f32(beta, "beta")
    lib = _lib.load()
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    _rows(frames, "warp_gram_rhs_lists", "frames")
    nslot = layout["nslot"]
    need = lib.dnmf_warp_gram_rhs_lists_workspace(nslot, K, X, Y, Z, B)
    workspace = _workspace(workspace, need, dev)
    G, r = _gram_out(out, B, K, dev, "warp_gram_rhs_lists") if finish else (None, None)
    counters = None
    if TIMING is not None:
        if LISTS_COUNTERS is None:
            LISTS_COUNTERS = torch.zeros(12, dtype=torch.int64, device=dev)   # [2:] only in stamp builds
        counters = LISTS_COUNTERS
    with _timed("warp_gram_rhs_lists"):
        rc = lib.dnmf_warp_gram_rhs_lists(
            layout["At"].data_ptr(), layout["bbox"].data_ptr(), layout["pair_slot"].data_ptr(),
            layout["axis_masks"].data_ptr(), nslot, K, X, Y, Z,
            beta.data_ptr(), beta.shape[2], _ptr(tt), B, frames.data_ptr(), frames.stride(0), _ptr(fid), _ptr(G),
            _ptr(r), workspace.data_ptr(), _nbytes(workspace), _ptr(counters), *_lists_form(passes, chunks), _stream())
    _lib.check(rc, "dnmf_warp_gram_rhs_lists")
    return G, r, workspace


def mu_temporal_slots(layout, workspace, sz, C, iters: int, passes=None, chunks=None):
    """K4 straight from the slot tables ``warp_gram_rhs_lists(..., finish=False)`` left in ``workspace``; C (K,T) fp32
    updated in place (T = the frames of that launch, ``passes`` and ``chunks`` those of that launch).  Needs ``layout["nbr"]``."""
    _state("mu_temporal_slots", C, torch.float32)
    K, T = C.shape
    lib = _lib.load()
    nbr = layout["nbr"]
    with _timed("mu_temporal_slots"):
        rc = lib.dnmf_mu_temporal_slots(workspace.data_ptr(), _lists_tables(sz, T, passes, chunks),
                                        layout["nslot"], layout["pair_slot"].data_ptr(), C.data_ptr(), C.stride(0), K, T,
                                        int(iters), nbr.data_ptr(), nbr.shape[1], _stream())
    _lib.check(rc, "dnmf_mu_temporal_slots")
    return C


def hals_temporal_slots(layout, workspace, sz, C, iters: int, kkt=False, passes=None, chunks=None):
    """K4h straight from the slot tables ``warp_gram_rhs_lists(..., finish=False)`` left in ``workspace``; C (K,T) fp32
    updated in place (T = the frames of that launch, ``passes`` and ``chunks`` those of that launch).  Needs
    ``layout["nbr"]``.  ``kkt`` as for ``hals_temporal``."""
    _state("hals_temporal_slots", C, torch.float32)
    if int(iters) < 0:
        raise ValueError(f"hals_temporal_slots: iters={iters} < 0")
    K, T = C.shape
    nbr = layout["nbr"]
    if nbr is None:
        raise ValueError("hals_temporal_slots: the layout has no neighbour lists (pattern wider than 32 columns)")
    lib = _lib.load()
    out = torch.empty((T,), dtype=torch.float64, device=C.device) if kkt else None
    with _timed("hals_temporal_slots"):
        rc = lib.dnmf_hals_temporal_slots(workspace.data_ptr(), _lists_tables(sz, T, passes, chunks),
                                          layout["nslot"], layout["pair_slot"].data_ptr(), C.data_ptr(), C.stride(0), K, T,
                                          int(iters), nbr.data_ptr(), nbr.shape[1], _ptr(out), _stream())
    _lib.check(rc, "dnmf_hals_temporal_slots")
    return (C, out) if kkt else C


class Communicator:
    """C1: the library's RCCL communicator over the ranks of a ``torch.distributed`` group (one process per GPU).

    ``torch.distributed`` is only the out-of-band channel for the 128-byte id; the all-reduce itself is
    ``dnmf_allreduce_sum_f32`` on torch's current stream.  ``group=None`` with no initialised default group gives a
    one-rank communicator."""

    def __init__(self, group=None):
        import torch.distributed as dist
        lib = _lib.load()
        multi = dist.is_available() and dist.is_initialized()
        self.nranks = dist.get_world_size(group) if multi else 1
        self.rank = dist.get_rank(group) if multi else 0
        ident = ctypes.create_string_buffer(128)
        if self.rank == 0:
            _lib.check(lib.dnmf_comm_unique_id(ident), "dnmf_comm_unique_id")
        if self.nranks > 1:
            on_gpu = dist.get_backend(group) == "nccl"
            t = torch.frombuffer(bytearray(ident.raw), dtype=torch.uint8).clone()
            t = t.cuda() if on_gpu else t
            dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            ident = ctypes.create_string_buffer(bytes(t.cpu().tolist()), 128)
        handle = ctypes.c_void_p()
        _lib.check(lib.dnmf_comm_init(ctypes.byref(handle), ident, self.nranks, self.rank), "dnmf_comm_init")
        self._handle = handle

    def all_reduce_(self, t: torch.Tensor) -> torch.Tensor:
        """In-place sum over ranks of a contiguous fp32 CUDA tensor."""
        t = _f32(t, "all_reduce_")
        with _timed("allreduce"):
            rc = _lib.load().dnmf_allreduce_sum_f32(self._handle, _ptr(t), t.numel(), _stream())
        _lib.check(rc, "dnmf_allreduce_sum_f32")
        return t

    def close(self):
        if self._handle:
            _lib.check(_lib.load().dnmf_comm_destroy(self._handle), "dnmf_comm_destroy")
            self._handle = None


def image_iwarp(frames, frame_ids, sz, beta, times, out=None, exhaustive=False, count=None, nchan=1):
    """K7.  Registered frames (B,P): nearest-neighbour inverse warp under beta[:, :, times].  ``exhaustive``: search
    all P candidates for every lattice point (the checker of the window search); ``count``: int64[1] CUDA tensor
    incremented by the lattice points that needed the exhaustive search.  ``nchan`` > 1: a frame row holds that many
    channels of P floats that share the warp (MultiChannelDNMF), one search per lattice point serves all of them
    (``dnmf_image_iwarp_channels``) and the result is (B, nchan*P)."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    nchan = int(nchan)
    if nchan < 1:
        raise ValueError(f"image_iwarp: nchan={nchan}")
    _f32(beta, "beta")
    _rows(frames, "image_iwarp", "frames")
    if nchan > 1 and frames.shape[-1] < nchan * P:
        raise ValueError(f"image_iwarp: rows of {frames.shape[-1]} floats cannot hold {nchan} channels of {P}")
    dev = frames.device
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    if out is None:
        out = torch.empty((B, nchan * P), dtype=torch.float32, device=dev)
    if out.shape[0] < B or out.stride(0) < nchan * P or out.stride(1) != 1:
        raise ValueError(f"image_iwarp: out must be (>=B, ld) with ld >= {nchan} x P")
    lib = _lib.load()
    # frames per launch (gridDim.y); one flag byte per lattice point of the launch: at most 256 MiB of flags (a 512x512x20
    # volume would otherwise ask for 86 GB per 16384-frame launch)
    step = max(1, min(16384, (256 << 20) // P))
    ws = torch.empty((lib.dnmf_image_iwarp_workspace(X, Y, Z, min(B, step)),), dtype=torch.uint8, device=dev)
    for s in range(0, B, step):
        n = min(step, B - s)
        src = frames if fid is not None else frames[s:]   # without ids, frame b of a launch is its row b
        with _timed("image_iwarp"):
            if nchan == 1:
                rc = (lib.dnmf_image_iwarp(src.data_ptr(), frames.stride(0), 0 if fid is None else fid[s:].data_ptr(), X, Y, Z,
                                            beta.data_ptr(), beta.shape[2], tt[s:].data_ptr(), n, out[s:].data_ptr(),
                                            out.stride(0), ws.data_ptr(), ws.numel(), int(bool(exhaustive)), _ptr(count),
                                            _stream()))
            else:
                rc = (lib.dnmf_image_iwarp_channels(src.data_ptr(), frames.stride(0), P, nchan,
                                                     0 if fid is None else fid[s:].data_ptr(), X, Y, Z, beta.data_ptr(),
                                                     beta.shape[2], tt[s:].data_ptr(), n, out[s:].data_ptr(), out.stride(0), P,
                                                     ws.data_ptr(), ws.numel(), int(bool(exhaustive)), _ptr(count), _stream()))
        _lib.check(rc, "dnmf_image_iwarp")
    return out


PULLBACK_MAX_FRAMES = 32768   # frames per K17 launch (they ride on gridDim.y)


def warp_pullback(frames, frame_ids, sz, beta, times, out=None, nchan=1, fill=None, coords=None, count=None):
    """K17.  Registered frames (B, nchan*P): for every lattice point u of the volume the x with q_t(x) = u under
    beta[:, :, times] (Newton from u), and the frame sampled trilinearly there (zero padding, the model's own forward).  True
    voxel coordinates: none of the reference's ``sz``-for-``sz - 1`` scaling that K7 (``image_iwarp``) keeps -- an extension,
    not a parity path.  ``frames`` / ``frame_ids`` / ``times`` / ``out`` / ``nchan`` as ``image_iwarp`` (``times`` None:
    column b of beta for frame b).  ``fill``: None = zero padding, points without a solution get 0; a float (NaN, say) is
    written to every point whose x lies outside the volume and to points without a solution.  ``coords``: a (B,P,3) fp32 CUDA
    tensor that receives x (NaN where there is no solution); ``count``: int64[1] CUDA tensor incremented by the lattice
    points without a solution."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    nchan = int(nchan)
    if nchan < 1:
        raise ValueError(f"warp_pullback: nchan={nchan}")
    _f32(beta, "beta")
    if beta.dim() != 3 or tuple(beta.shape[:2]) != (10, 3):
        raise ValueError(f"warp_pullback: beta must be (10,3,T), got {tuple(beta.shape)}")
    _rows(frames, "warp_pullback", "frames", nchan * P, f" and rows of {nchan} x {P} floats")
    dev = frames.device
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    if out is None:
        out = torch.empty((B, nchan * P), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or not out.is_cuda or out.dim() != 2 or out.shape[0] < B or out.stride(0) < nchan * P or out.stride(1) != 1:
        raise ValueError(f"warp_pullback: out must be float32 CUDA (>=B, ld) with ld >= {nchan} x P")
    if coords is not None and (coords.dtype != torch.float32 or not coords.is_cuda or not coords.is_contiguous()
                               or tuple(coords.shape) != (B, P, 3)):
        raise ValueError(f"warp_pullback: coords must be a contiguous float32 CUDA tensor of shape ({B}, {P}, 3)")
    if count is not None and (count.dtype != torch.int64 or not count.is_cuda or count.numel() < 1):
        raise ValueError("warp_pullback: count must be an int64 CUDA tensor")
    if tt is None:
        tt = torch.arange(B, dtype=torch.int32, device=dev)
    # the row stride of a single row means nothing (a view through numpy's newaxis has 0)
    ldf = frames.stride(0) if frames.shape[0] != 1 else max(frames.stride(0), nchan * P)
    lib = _lib.load()
    for s in range(0, B, PULLBACK_MAX_FRAMES):
        n = min(PULLBACK_MAX_FRAMES, B - s)
        src = frames if fid is not None else frames[s:]   # without ids, frame b of a launch is its row b
        with _timed("warp_pullback"):
            rc = lib.dnmf_warp_pullback(src.data_ptr(), ldf, P, nchan, 0 if fid is None else fid[s:].data_ptr(), X, Y, Z,
                                        beta.data_ptr(), beta.shape[2], tt[s:].data_ptr(), n, out[s:].data_ptr(), out.stride(0), P,
                                        0 if fill is None else 1,
                                        0.0 if fill is None else float(fill), 0 if coords is None else coords[s:].data_ptr(),
                                        _ptr(count), _stream())
        _lib.check(rc, "dnmf_warp_pullback")
    return out


def nearest_points(points, queries, values=None, out_index=None, out=None, _workspace_bytes=None):
    """K10.  points (B,N,3) fp32 or fp64 CUDA, queries (Q,3) (one set for every frame) or (B,Q,3), converted to float64 ->
    ``index`` (B,Q) int32: per frame and query the point of the smallest float64 (d2, index), exact, ties to the lowest index;
    with ``values`` (B,N) fp32 also ``vals`` (B,Q) = values[b][index], returned as ``(index, vals)``.  ``out_index`` /
    ``out``: (B,Q) outputs to fill (row strides allowed).  Raises ValueError on a non-finite point or query.
    ``_workspace_bytes``: a smaller workspace than the call's 512 MiB chunk (tests: several chunks of frames per call)."""
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype in (torch.float32, torch.float64)
            and points.dim() == 3 and points.shape[2] == 3):
        raise ValueError("nearest_points: points must be a (B,N,3) float32 or float64 CUDA tensor")
    dev = points.device
    B, N = points.shape[0], points.shape[1]
    if N < 1:
        raise ValueError("nearest_points: need at least one point per frame")
    if points.stride(2) != 1 or points.stride(1) != 3:
        points = points.contiguous()
    q = torch.as_tensor(queries).to(device=dev, dtype=torch.float64)
    if q.dim() not in (2, 3) or q.shape[-1] != 3 or (q.dim() == 3 and q.shape[0] != B):
        raise ValueError(f"nearest_points: queries must be (Q,3) or ({B},Q,3), got {tuple(q.shape)}")
    q = q.contiguous()
    Q = q.shape[-2]
    if not bool(torch.isfinite(points).all()) or not bool(torch.isfinite(q).all()):
        raise ValueError("nearest_points: points and queries must be finite")
    if out_index is None:
        out_index = torch.empty((B, Q), dtype=torch.int32, device=dev)
    if (out_index.dtype != torch.int32 or not out_index.is_cuda or out_index.dim() != 2 or out_index.shape[0] < B
            or out_index.shape[1] < Q or (Q > 1 and out_index.stride(1) != 1)):
        raise ValueError("nearest_points: out_index must be int32 CUDA (>=B, >=Q) with unit inner stride")
    if values is not None:
        if (values.dtype != torch.float32 or not values.is_cuda or values.dim() != 2 or values.shape[0] < B
                or values.shape[1] != N or (N > 1 and values.stride(1) != 1)):
            raise ValueError(f"nearest_points: values must be float32 CUDA ({B},{N}) with unit inner stride")
        if out is None:
            out = torch.empty((B, Q), dtype=torch.float32, device=dev)
        if (out.dtype != torch.float32 or not out.is_cuda or out.dim() != 2 or out.shape[0] < B or out.shape[1] < Q
                or (Q > 1 and out.stride(1) != 1)):
            raise ValueError("nearest_points: out must be float32 CUDA (>=B, >=Q) with unit inner stride")
    if B == 0 or Q == 0:
        return out_index if values is None else (out_index, out)
    lib = _lib.load()
    need = lib.dnmf_nearest_points_workspace(N, B)
    if _workspace_bytes is not None:
        need = min(need, max(int(_workspace_bytes), lib.dnmf_nearest_points_workspace(N, 1)))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    with _timed("nearest_points"):
        rc = lib.dnmf_nearest_points(points.data_ptr(), int(points.dtype == torch.float64), points.stride(0), N, q.data_ptr(),
                                     0 if q.dim() == 2 else q.stride(0), Q, B, _ptr(values),
                                     0 if values is None else values.stride(0), out_index.data_ptr(), out_index.stride(0),
                                     _ptr(out), Q if out is None else out.stride(0), ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "dnmf_nearest_points")
    return out_index if values is None else (out_index, out)


def patch_grid(sz, strides, overlaps):
    """The patch grid of the reference's ``sliding_window_3d`` (MotionCorrect.py:1190-1221): ``(dims (3,), starts (NP,3))`` as
    numpy int arrays, patches in the reference's order (x outermost)."""
    import numpy as np
    X, Y, Z = (int(s) for s in sz)
    st = _int3(strides)
    ov = _int3(overlaps)
    dims = (ctypes.c_int * 3)()
    lib = _lib.load()
    NP = lib.dnmf_register_patches_grid(X, Y, Z, st, ov, dims, None)
    if NP <= 0:
        raise ValueError(f"patch_grid: windows of strides {tuple(strides)} + overlaps {tuple(overlaps)} do not fit the volume {X}x{Y}x{Z}")
    starts = (ctypes.c_int * (3 * NP))()
    lib.dnmf_register_patches_grid(X, Y, Z, st, ov, dims, starts)
    return np.array(list(dims)), np.array(list(starts)).reshape(NP, 3)


def register_patches(frames, tmpl, sz, strides, overlaps, max_shifts, max_deviation_rigid=3, upsample_factor=10,
                     add_to_movie=0.0, frame_ids=None, valu=None):
    """K8.  frames (>=B, P) fp32 CUDA rows, tmpl (P) -> rigid shifts (B,3) and per-patch shifts (B,NP,3) (signs -x, -y, +z:
    the reference's ``x/y/z_shifts_els``).  ``valu``: the vector-ALU axis kernel instead of the MFMA one (None: ``K8_VALU``)."""
    X, Y, Z = (int(s) for s in sz)
    _rows(frames, "register_patches", "frames")
    dev = frames.device
    tm = _f32(tmpl.reshape(-1), "tmpl")
    fid, _, B = _ids(frames, frame_ids, None, dev)
    st = _int3(strides)
    ov = _int3(overlaps)
    ms = _int3(max_shifts)
    lib = _lib.load()
    NP = lib.dnmf_register_patches_grid(X, Y, Z, st, ov, None, None)
    if NP <= 0:
        raise ValueError(f"register_patches: windows of strides {tuple(strides)} + overlaps {tuple(overlaps)} do not fit the volume")
    need = lib.dnmf_register_patches_workspace(X, Y, Z, st, ov, B)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    rigid = torch.empty((B, 3), dtype=torch.float32, device=dev)
    patch = torch.empty((B, NP, 3), dtype=torch.float32, device=dev)
    with _timed("register_patches"):
        rc = lib.dnmf_register_patches(frames.data_ptr(), frames.stride(0), _ptr(fid), B, tm.data_ptr(), X, Y, Z, st, ov, ms,
                                       int(max_deviation_rigid), int(upsample_factor), float(add_to_movie), rigid.data_ptr(),
                                       patch.data_ptr(), ws.data_ptr(), ws.numel(), int(K8_VALU if valu is None else valu), _stream())
    _lib.check(rc, "dnmf_register_patches")
    return rigid, patch


_BORDER = {False: 0, True: 1, 'min': 2, 'copy': 3}     # border_nan of apply_shifts_dft (MotionCorrect.py:1098-1145)


def rigid_correct(frames, tmpl, sz, max_shifts, upsample_factor=10, add_to_movie=0.0, border_nan=True, frame_ids=None,
                  want_frames=False, tsum=None, tcount=None, valu=None):
    """K8, rigid pass.  frames (>=B, P) fp32 CUDA rows, tmpl (P) -> (rigid shifts (B,3) as register_translation_3d returns
    them, corrected frames (B,P) or None, tsum (P) fp32, tcount (P) int32): the per-voxel sums and counts of the finite
    corrected values are ADDED into ``tsum`` / ``tcount`` when given (a video walked in pieces), else start from zero.
    ``valu`` as for ``register_patches``."""
    X, Y, Z = (int(s) for s in sz)
    _rows(frames, "rigid_correct", "frames")
    dev = frames.device
    P = X * Y * Z
    tm = _f32(tmpl.reshape(-1), "tmpl")
    fid, _, B = _ids(frames, frame_ids, None, dev)
    ms = _int3(max_shifts)
    lib = _lib.load()
    ws = torch.empty((lib.dnmf_rigid_correct_workspace(X, Y, Z, B),), dtype=torch.uint8, device=dev)
    rigid = torch.empty((B, 3), dtype=torch.float32, device=dev)
    out = torch.empty((B, P), dtype=torch.float32, device=dev) if want_frames else None
    if tsum is None:
        tsum, tcount = torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    with _timed("rigid_correct"):
        rc = lib.dnmf_rigid_correct(frames.data_ptr(), frames.stride(0), _ptr(fid), B, tm.data_ptr(), X, Y, Z, ms,
                                    int(upsample_factor), float(add_to_movie), _BORDER[border_nan], rigid.data_ptr(),
                                    _ptr(out), P, tsum.data_ptr(), tcount.data_ptr(), ws.data_ptr(), ws.numel(),
                                    int(K8_VALU if valu is None else valu), _stream())
    _lib.check(rc, "dnmf_rigid_correct")
    return rigid, out, tsum, tcount


def apply_pwrigid(frames, patch_shifts, sz, strides, overlaps, add_to_movie=0.0, frame_ids=None, out=None, tsum=None, tcount=None):
    """K9.  frames (>=B, P) fp32 CUDA rows, patch_shifts (B,NP,3) with the signs of x/y/z_shifts_els (-x, -y, +z) -> (the
    piecewise-rigid corrected frames out (B,P) (or (>=B, ldo) given), tsum (P) fp32, tcount (P) int32): the per-voxel sums and
    counts of the finite corrected values are ADDED into ``tsum`` / ``tcount`` when given, else start from zero."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    _rows(frames, "apply_pwrigid", "frames")
    dev = frames.device
    sh = _f32(patch_shifts, "patch_shifts")
    fid, _, B = _ids(frames, frame_ids, None, dev)
    st = _int3(strides)
    ov = _int3(overlaps)
    lib = _lib.load()
    NP = lib.dnmf_register_patches_grid(X, Y, Z, st, ov, None, None)
    if NP <= 0:
        raise ValueError(f"apply_pwrigid: windows of strides {tuple(strides)} + overlaps {tuple(overlaps)} do not fit the volume")
    if tuple(sh.shape) != (B, NP, 3):
        raise ValueError(f"apply_pwrigid: patch_shifts must be ({B}, {NP}, 3), got {tuple(sh.shape)}")
    if out is None:
        out = torch.empty((B, P), dtype=torch.float32, device=dev)
    if out.shape[0] < B or out.stride(0) < P or out.stride(1) != 1 or out.dtype != torch.float32:
        raise ValueError("apply_pwrigid: out must be float32 (>=B, ld) with ld >= P")
    if tsum is None:
        tsum, tcount = torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    ws = torch.empty((lib.dnmf_apply_pwrigid_workspace(X, Y, Z, st, ov, B),), dtype=torch.uint8, device=dev)
    with _timed("apply_pwrigid"):
        rc = lib.dnmf_apply_pwrigid(frames.data_ptr(), frames.stride(0), _ptr(fid), B, X, Y, Z, st, ov, sh.data_ptr(),
                                    float(add_to_movie), out.data_ptr(), out.stride(0), tsum.data_ptr(), tcount.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "dnmf_apply_pwrigid")
    return out, tsum, tcount


def apply_shifts_points(points, patch_shifts, centers):
    """points (K,3), patch_shifts (T,NP,3), centers (NP,3) -> (K,3,T) fp32 (MotionCorrect.apply_shifts_points)."""
    pts, sh, ce = _f32(points, "points"), _f32(patch_shifts, "patch_shifts"), _f32(centers, "centers")
    K, (T, NP, _) = pts.shape[0], sh.shape
    out = torch.empty((K, 3, T), dtype=torch.float32, device=pts.device)
    _lib.check(_lib.load().dnmf_apply_shifts_points(pts.data_ptr(), K, sh.data_ptr(), T, NP, ce.data_ptr(), out.data_ptr(), _stream()),
               "dnmf_apply_shifts_points")
    return out


WARP_ORDERS = {"translation": 0, "affine": 1, "quadratic": 2}


def warp_free_rows(sz, order):
    """Rows of beta that ``fit_quadratic_warp`` fits: those of ``order`` without every row that involves an axis of extent 1."""
    rows = {"translation": [0], "affine": [0, 1, 2, 3], "quadratic": list(range(10))}[order]
    for d, uses in enumerate(((1, 4, 7, 8), (2, 5, 7, 9), (3, 6, 8, 9))):
        if int(sz[d]) == 1:
            rows = [r for r in rows if r not in uses]
    return rows


def _tracks(P, name):
    """(K,3,T) float32 or float64 CUDA, contiguous."""
    if not (isinstance(P, torch.Tensor) and P.is_cuda and P.dtype in (torch.float32, torch.float64) and P.dim() == 3
            and P.shape[1] == 3):
        raise ValueError(f"{name}: tracks must be a (K,3,T) float32 or float64 CUDA tensor")
    if P.shape[0] < 1 or P.shape[2] < 1:
        raise ValueError(f"{name}: tracks of shape {tuple(P.shape)}: need K >= 1 and T >= 1")
    return P.contiguous()


def fit_quadratic_warp(P, targets, sz, order="quadratic", ridge=0.0):
    """K11.  P (K,3,T) fp32 / fp64 CUDA tracks (NaN = neuron k not tracked in frame t), targets (K,3) -> ``(beta (10,3,T)
    fp32, ok (T) bool)``: per frame the least-squares beta_t with q_t(P[k,:,t]) = targets[k] over the free rows of ``order``
    ('translation', 'affine', 'quadratic'), pulled to the identity by ``ridge`` (see include/dnmf_hip.h).  Frames whose
    system is singular get the identity and ok = False.  ValueError when ridge == 0 and every frame has fewer tracked
    neurons than free rows."""
    if order not in WARP_ORDERS:
        raise ValueError(f"fit_quadratic_warp: order must be one of {sorted(WARP_ORDERS)}, got {order!r}")
    if not (float(ridge) >= 0.0 and float(ridge) != float("inf")):
        raise ValueError(f"fit_quadratic_warp: ridge={ridge} must be >= 0 and finite")
    P = _tracks(P, "fit_quadratic_warp")
    K, _, T = P.shape
    X, Y, Z = (int(s) for s in sz)
    R = torch.as_tensor(targets).to(device=P.device, dtype=torch.float64).contiguous()
    if tuple(R.shape) != (K, 3):
        raise ValueError(f"fit_quadratic_warp: targets must be ({K}, 3), got {tuple(R.shape)}")
    if ridge == 0:
        nfree = len(warp_free_rows((X, Y, Z), order))
        most = int(torch.isfinite(P).all(1).sum(0).max())
        if most < nfree:
            raise ValueError(f"fit_quadratic_warp: at most {most} tracked neurons per frame for {nfree} free rows "
                             f"(order={order!r}) and ridge = 0")
    beta = torch.empty((10, 3, T), dtype=torch.float32, device=P.device)
    ok = torch.empty((T,), dtype=torch.uint8, device=P.device)
    with _timed("fit_quadratic_warp"):
        rc = _lib.load().dnmf_fit_quadratic_warp(P.data_ptr(), int(P.dtype == torch.float64), K, T, R.data_ptr(), X, Y, Z,
                                                 WARP_ORDERS[order], float(ridge), beta.data_ptr(), ok.data_ptr(), _stream())
    _lib.check(rc, "dnmf_fit_quadratic_warp")
    return beta, ok.bool()


def invert_quadratic_warp(beta, targets, times=None, start=None, tol=1e-6):
    """K12.  beta (10,3,T) fp32 CUDA, targets (K,3) -> (K,3,B) fp64 CUDA: for every neuron and every frame of ``times`` (None:
    all T) the x* with q_t(x*) = targets[k], by Newton's method from ``start`` (K,3,B) (None: the target); NaN where it did
    not converge within 32 steps or met a vanishing Jacobian."""
    beta = _f32(beta, "beta")
    if beta.dim() != 3 or tuple(beta.shape[:2]) != (10, 3):
        raise ValueError(f"invert_quadratic_warp: beta must be (10,3,T), got {tuple(beta.shape)}")
    T = beta.shape[2]
    dev = beta.device
    R = torch.as_tensor(targets).to(device=dev, dtype=torch.float64).contiguous()
    if R.dim() != 2 or R.shape[1] != 3 or R.shape[0] < 1:
        raise ValueError(f"invert_quadratic_warp: targets must be (K,3) with K >= 1, got {tuple(R.shape)}")
    K = R.shape[0]
    tt = None
    if times is not None:
        tt = _i32(times, dev)
        if tt.numel() and (int(tt.min()) < 0 or int(tt.max()) >= T):
            raise ValueError(f"invert_quadratic_warp: times outside [0, {T})")
    B = T if tt is None else tt.numel()
    if not float(tol) > 0.0:
        raise ValueError(f"invert_quadratic_warp: tol={tol} must be positive")
    st = None
    if start is not None:
        st = torch.as_tensor(start).to(device=dev, dtype=torch.float64).contiguous()
        if tuple(st.shape) != (K, 3, B):
            raise ValueError(f"invert_quadratic_warp: start must be ({K}, 3, {B}), got {tuple(st.shape)}")
    out = torch.empty((K, 3, B), dtype=torch.float64, device=dev)
    with _timed("invert_quadratic_warp"):
        rc = _lib.load().dnmf_invert_quadratic_warp(beta.data_ptr(), T, _ptr(tt), B, R.data_ptr(), K, _ptr(st), float(tol),
                                                    out.data_ptr(), _stream())
    _lib.check(rc, "dnmf_invert_quadratic_warp")
    return out


def roi_signals(frames, sz, P, window=(3, 3, 0)):
    """K13.  frames (T, ld >= X Y Z) fp32 CUDA rows (row t = frame t; ``ResidentLoader.frames_2d()`` /
    ``device_frames()``), P (K,3,T) fp32 / fp64 CUDA tracks -> (K,T) fp64 CUDA: the reference's ``get_roi_signals`` -- the
    mean of the box of 2 window + 1 voxels per axis around the rounded position, zeros outside the volume, NaN voxels left
    out, NaN for a position outside the volume."""
    X, Y, Z = (int(s) for s in sz)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2
            and frames.stride(1) == 1 and frames.stride(0) >= X * Y * Z and frames.shape[1] >= X * Y * Z):
        raise ValueError("roi_signals: frames must be float32 CUDA (T, ld) rows with unit inner stride and ld >= X Y Z")
    P = _tracks(P, "roi_signals")
    K, _, T = P.shape
    if frames.shape[0] < T:
        raise ValueError(f"roi_signals: {frames.shape[0]} frames for tracks of {T} frames")
    w = [int(v) for v in window]
    if len(w) != 3 or min(w) < 0:
        raise ValueError(f"roi_signals: window must be three integers >= 0, got {window}")
    out = torch.empty((K, T), dtype=torch.float64, device=frames.device)
    with _timed("roi_signals"):
        rc = _lib.load().dnmf_roi_signals(frames.data_ptr(), frames.stride(0), X, Y, Z, P.data_ptr(), int(P.dtype == torch.float64),
                                          K, T, _int3(w), out.data_ptr(), _stream())
    _lib.check(rc, "dnmf_roi_signals")
    return out


def detect_neurons(image, sz, K, shape_std=3, min_distance=None, threshold=0.0, background=None, workspace=None):
    """K14.  image: X Y Z float32 CUDA values (any shape with that many, voxel order of a frame row) -> ``(positions (K,3)
    fp32, amplitudes (K,) fp32, count (0-dim int32))`` on the device: the centres of up to K blobs exp(-|x - p|^2 /
    shape_std^2) by a greedy matched-filter pursuit (include/dnmf_hip.h), brightest first; rows from ``count`` on are NaN.
    ``min_distance`` (None: 2 shape_std): no two centres are closer; a pick must score above ``threshold``; ``background``
    (None: the image's median) is subtracted first."""
    X, Y, Z = (int(s) for s in sz)
    _f32(image, "image")
    if image.numel() != X * Y * Z:
        raise ValueError(f"detect_neurons: image of {image.numel()} values for a volume {X}x{Y}x{Z}")
    sigma, K = float(shape_std), int(K)
    if not (sigma > 0.0 and sigma != float("inf")):
        raise ValueError(f"detect_neurons: shape_std={shape_std} must be positive and finite")
    if K < 1:
        raise ValueError(f"detect_neurons: K={K} must be at least 1")
    md = 2.0 * sigma if min_distance is None else float(min_distance)
    bg = float(image.median()) if background is None else float(background)
    dev = image.device
    lib = _lib.load()
    need = _need(lib, "dnmf_detect_neurons_workspace", _int3((X, Y, Z)), K, sigma)
    workspace = _workspace(workspace, need, dev)
    positions = torch.empty((K, 3), dtype=torch.float32, device=dev)
    amplitudes = torch.empty((K,), dtype=torch.float32, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    with _timed("detect_neurons"):
        rc = lib.dnmf_detect_neurons(image.data_ptr(), _int3((X, Y, Z)), K, sigma, md, float(threshold), bg, positions.data_ptr(),
                                     amplitudes.data_ptr(), count.data_ptr(), workspace.data_ptr(), _nbytes(workspace), _stream())
    _lib.check(rc, "dnmf_detect_neurons")
    return positions, amplitudes, count


def track_neurons(frames, sz, predict, shape_std=3, search=(6, 6, 1), threshold=0.0, background=None, times=None):
    """K15.  frames (rows, ld >= X Y Z) fp32 CUDA rows (``ResidentLoader.frames_2d()`` / ``device_frames()``), predict (K,3,T)
    or (K,3) (used for every frame) fp32 / fp64 CUDA -> ``(positions (K,3,T) fp64, amplitudes (K,T) fp32, peaks (K,T) fp32)``
    on the device: for every neuron and every frame of ``times`` (None: rows 0..T-1; T = the frames of ``predict``, else every
    row) the sub-voxel peak of the frame's K14 score -- the matched filter with exp(-|x - p|^2 / shape_std^2), noise-normalised
    -- inside the window of ``search`` voxels per axis around the rounded prediction, its least-squares amplitude and the score
    at the picked voxel (include/dnmf_hip.h).  NaN where the prediction is not finite, the window misses the volume or the
    peak is not above ``threshold``.  ``background``: None (0), a number, or T values taken off the frames first.  The K T
    searches are independent and nothing is subtracted: a neuron within about 2 shape_std of a brighter one can be captured
    by it; ``search`` is the guard."""
    X, Y, Z = (int(s) for s in sz)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2
            and frames.stride(1) == 1 and frames.stride(0) >= X * Y * Z and frames.shape[1] >= X * Y * Z):
        raise ValueError("track_neurons: frames must be float32 CUDA (T, ld) rows with unit inner stride and ld >= X Y Z")
    dev = frames.device
    per_frame = isinstance(predict, torch.Tensor) and predict.dim() == 3
    if per_frame:
        predict = _tracks(predict, "track_neurons")
    elif not (isinstance(predict, torch.Tensor) and predict.is_cuda and predict.dtype in (torch.float32, torch.float64)
              and predict.dim() == 2 and predict.shape[1] == 3 and predict.shape[0] >= 1):
        raise ValueError("track_neurons: predict must be a (K,3,T) or (K,3) float32 or float64 CUDA tensor with K >= 1")
    predict = predict.contiguous()
    K = predict.shape[0]
    tt = None
    if times is not None:
        tt = _i32(times, dev)
        if tt.numel() < 1 or int(tt.min()) < 0 or int(tt.max()) >= frames.shape[0]:
            raise ValueError(f"track_neurons: times must be at least one row index in [0, {frames.shape[0]})")
    T = tt.numel() if tt is not None else (predict.shape[2] if per_frame else frames.shape[0])
    if per_frame and predict.shape[2] != T:
        raise ValueError(f"track_neurons: predict of {predict.shape[2]} frames for {T} frames")
    if tt is None and frames.shape[0] < T:
        raise ValueError(f"track_neurons: {frames.shape[0]} frames for a prediction of {T} frames")
    w = [int(v) for v in search]
    if len(w) != 3 or min(w) < 0:
        raise ValueError(f"track_neurons: search must be three integers >= 0, got {search}")
    sigma = float(shape_std)
    if not (sigma > 0.0 and sigma != float("inf")):
        raise ValueError(f"track_neurons: shape_std={shape_std} must be positive and finite")
    bg = None
    if background is not None:
        if isinstance(background, torch.Tensor) or hasattr(background, "__len__"):
            bg = torch.as_tensor(background).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if bg.numel() != T:
                raise ValueError(f"track_neurons: background of {bg.numel()} values for {T} frames")
        else:
            bg = torch.full((T,), float(background), dtype=torch.float32, device=dev)
    positions = torch.empty((K, 3, T), dtype=torch.float64, device=dev)
    amplitudes = torch.empty((K, T), dtype=torch.float32, device=dev)
    peaks = torch.empty((K, T), dtype=torch.float32, device=dev)
    with _timed("track_neurons"):
        rc = _lib.load().dnmf_track_neurons(frames.data_ptr(), frames.stride(0), _int3((X, Y, Z)), T, _ptr(tt), predict.data_ptr(),
                                            int(predict.dtype == torch.float64), int(per_frame), K, sigma, _int3(w), float(threshold),
                                            _ptr(bg), positions.data_ptr(), amplitudes.data_ptr(), peaks.data_ptr(), _stream())
    _lib.check(rc, "dnmf_track_neurons")
    return positions, amplitudes, peaks


def track_neurons_exclusive(frames, sz, predict, order, shape_std=3, search=(6, 6, 1), rounds=2, threshold=0.0, background=None,
                            times=None):
    """K15x.  ``track_neurons`` with exclusion between the neurons of a frame: frames, predict, shape_std, search, threshold,
    background, times as there, order (K,T) int32 CUDA, a permutation of 0..K-1 per frame -> ``(positions (K,3,T) fp64,
    amplitudes (K,T) fp32, peaks (K,T) fp32, n_subtracted (K,T) int32)``.  Per frame the neurons are searched in the sequence
    ``order[:, t]``, each on the frame less the model footprints -- amplitude x exp(-|x - p^|^2 / shape_std^2) within
    ceil(3 shape_std) voxels of the pick -- of the neurons already placed in that frame, so a neuron within about 2 shape_std
    of a brighter one that is searched first is no longer captured by it; rounds 2 .. ``rounds`` search every neuron again
    with all others taken off at their latest result (include/dnmf_hip.h).  A neuron without a result is NaN and is not taken
    off.  ``n_subtracted``: the neighbours whose footprint met the searched region in the last round.  One workgroup per frame
    walks its K rounds searches in sequence; K <= 1024."""
    X, Y, Z = (int(s) for s in sz)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2
            and frames.stride(1) == 1 and frames.stride(0) >= X * Y * Z and frames.shape[1] >= X * Y * Z):
        raise ValueError("track_neurons_exclusive: frames must be float32 CUDA (T, ld) rows with unit inner stride and ld >= X Y Z")
    dev = frames.device
    per_frame = isinstance(predict, torch.Tensor) and predict.dim() == 3
    if per_frame:
        predict = _tracks(predict, "track_neurons_exclusive")
    elif not (isinstance(predict, torch.Tensor) and predict.is_cuda and predict.dtype in (torch.float32, torch.float64)
              and predict.dim() == 2 and predict.shape[1] == 3 and predict.shape[0] >= 1):
        raise ValueError("track_neurons_exclusive: predict must be a (K,3,T) or (K,3) float32 or float64 CUDA tensor with K >= 1")
    predict = predict.contiguous()
    K = predict.shape[0]
    tt = None
    if times is not None:
        tt = _i32(times, dev)
        if tt.numel() < 1 or int(tt.min()) < 0 or int(tt.max()) >= frames.shape[0]:
            raise ValueError(f"track_neurons_exclusive: times must be at least one row index in [0, {frames.shape[0]})")
    T = tt.numel() if tt is not None else (predict.shape[2] if per_frame else frames.shape[0])
    if per_frame and predict.shape[2] != T:
        raise ValueError(f"track_neurons_exclusive: predict of {predict.shape[2]} frames for {T} frames")
    if tt is None and frames.shape[0] < T:
        raise ValueError(f"track_neurons_exclusive: {frames.shape[0]} frames for a prediction of {T} frames")
    w = [int(v) for v in search]
    if len(w) != 3 or min(w) < 0:
        raise ValueError(f"track_neurons_exclusive: search must be three integers >= 0, got {search}")
    sigma = float(shape_std)
    if not (sigma > 0.0 and sigma != float("inf")):
        raise ValueError(f"track_neurons_exclusive: shape_std={shape_std} must be positive and finite")
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError(f"track_neurons_exclusive: rounds={rounds} must be at least 1")
    if not (isinstance(order, torch.Tensor) and order.is_cuda and order.dtype == torch.int32 and tuple(order.shape) == (K, T)):
        raise ValueError(f"track_neurons_exclusive: order must be a ({K}, {T}) int32 CUDA tensor")
    order = order.contiguous()
    if not bool((order.sort(dim=0).values == torch.arange(K, dtype=torch.int32, device=dev)[:, None]).all()):
        raise ValueError("track_neurons_exclusive: order must hold every neuron 0..K-1 once per frame (a permutation per column)")
    bg = None
    if background is not None:
        if isinstance(background, torch.Tensor) or hasattr(background, "__len__"):
            bg = torch.as_tensor(background).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if bg.numel() != T:
                raise ValueError(f"track_neurons_exclusive: background of {bg.numel()} values for {T} frames")
        else:
            bg = torch.full((T,), float(background), dtype=torch.float32, device=dev)
    positions = torch.empty((K, 3, T), dtype=torch.float64, device=dev)
    amplitudes = torch.empty((K, T), dtype=torch.float32, device=dev)
    peaks = torch.empty((K, T), dtype=torch.float32, device=dev)
    n_subtracted = torch.empty((K, T), dtype=torch.int32, device=dev)
    with _timed("track_neurons_exclusive"):
        rc = _lib.load().dnmf_track_neurons_exclusive(frames.data_ptr(), frames.stride(0), _int3((X, Y, Z)), T, _ptr(tt), predict.data_ptr(),
                                                      int(predict.dtype == torch.float64), int(per_frame), K, order.data_ptr(), rounds,
                                                      sigma, _int3(w), float(threshold), _ptr(bg), positions.data_ptr(),
                                                      amplitudes.data_ptr(), peaks.data_ptr(), n_subtracted.data_ptr(), _stream())
    _lib.check(rc, "dnmf_track_neurons_exclusive")
    return positions, amplitudes, peaks, n_subtracted


def follow_neurons(frames, sz, start, shape_std=3, search=(3, 3, 1), anchor=0, momentum=0.0, max_gap=5, threshold=0.0, background=None,
                   times=None):
    """K15c.  frames as ``track_neurons`` takes them, start (K,3) fp32 / fp64 CUDA: the centres in frame ``anchor`` -> a dict of
    CUDA tensors ``positions (K,3,T) fp64, amplitudes (K,T) fp32, peaks (K,T) fp32, predicted (K,3,T) fp64, lost_at (K,2)
    int32``: every neuron followed from the anchor frame to the last and to the first frame of ``times`` (None: every row;
    ``anchor`` counts its slots) by K15's search chained on itself (include/dnmf_hip.h): frame j is searched within ``search``
    voxels of ``predicted[k, :, j]`` = the last position found + ``momentum`` x the last step x the frames since.  A frame
    without a result is NaN and the chain coasts; after more than ``max_gap`` such frames in a row it is lost: ``lost_at[k]``
    (forward, backward) holds that frame (-1: never lost) and the frames after it are NaN.  A start row that is not finite gives
    NaN rows and ``lost_at = anchor``.  ``shape_std``, ``threshold``, ``background`` as in ``track_neurons``.  The T steps of a
    chain are sequential and only 2 K workgroups run; there is still no exclusion between neurons: a neuron within about
    2 shape_std of a brighter one can be captured by it, and both chains then follow the same blob."""
    X, Y, Z = (int(s) for s in sz)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2
            and frames.stride(1) == 1 and frames.stride(0) >= X * Y * Z and frames.shape[1] >= X * Y * Z):
        raise ValueError("follow_neurons: frames must be float32 CUDA (T, ld) rows with unit inner stride and ld >= X Y Z")
    dev = frames.device
    if not (isinstance(start, torch.Tensor) and start.is_cuda and start.dtype in (torch.float32, torch.float64) and start.dim() == 2
            and start.shape[1] == 3 and start.shape[0] >= 1):
        raise ValueError("follow_neurons: start must be a (K,3) float32 or float64 CUDA tensor with K >= 1")
    start = start.double().contiguous()
    K = start.shape[0]
    tt = None
    if times is not None:
        tt = _i32(times, dev)
        if tt.numel() < 1 or int(tt.min()) < 0 or int(tt.max()) >= frames.shape[0]:
            raise ValueError(f"follow_neurons: times must be at least one row index in [0, {frames.shape[0]})")
    T = tt.numel() if tt is not None else frames.shape[0]
    w = [int(v) for v in search]
    if len(w) != 3 or min(w) < 0:
        raise ValueError(f"follow_neurons: search must be three integers >= 0, got {search}")
    sigma = float(shape_std)
    if not (sigma > 0.0 and sigma != float("inf")):
        raise ValueError(f"follow_neurons: shape_std={shape_std} must be positive and finite")
    anchor, max_gap, momentum = int(anchor), int(max_gap), float(momentum)
    if not 0 <= anchor < T:
        raise ValueError(f"follow_neurons: anchor={anchor} outside [0, {T})")
    if not 0.0 <= momentum <= 1.0:
        raise ValueError(f"follow_neurons: momentum={momentum} must lie in [0, 1]")
    if max_gap < 0:
        raise ValueError(f"follow_neurons: max_gap={max_gap} must not be negative")
    bg = None
    if background is not None:
        if isinstance(background, torch.Tensor) or hasattr(background, "__len__"):
            bg = torch.as_tensor(background).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if bg.numel() != T:
                raise ValueError(f"follow_neurons: background of {bg.numel()} values for {T} frames")
        else:
            bg = torch.full((T,), float(background), dtype=torch.float32, device=dev)
    out = dict(positions=torch.empty((K, 3, T), dtype=torch.float64, device=dev),
               amplitudes=torch.empty((K, T), dtype=torch.float32, device=dev), peaks=torch.empty((K, T), dtype=torch.float32, device=dev),
               predicted=torch.empty((K, 3, T), dtype=torch.float64, device=dev), lost_at=torch.empty((K, 2), dtype=torch.int32, device=dev))
    with _timed("follow_neurons"):
        rc = _lib.load().dnmf_follow_neurons(frames.data_ptr(), frames.stride(0), _int3((X, Y, Z)), T, _ptr(tt), start.data_ptr(), K, sigma,
                                             _int3(w), anchor, momentum, max_gap, float(threshold), _ptr(bg), out["positions"].data_ptr(),
                                             out["amplitudes"].data_ptr(), out["peaks"].data_ptr(), out["predicted"].data_ptr(),
                                             out["lost_at"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_follow_neurons")
    return out


NEIGHBOURS = {"face": 0, "full": 1}   # DNMF_NEIGHBOURS_* of include/dnmf_hip.h


def summary_images_state(sz, B, neighbours='full', segment=0, device="cuda"):
    """An empty state for ``summary_images`` calls of up to ``B`` frames each (a movie fed in pieces whose first is not the
    largest); pass it with ``first=True``."""
    if neighbours not in NEIGHBOURS:
        raise ValueError(f"summary_images_state: neighbours must be 'face' or 'full', got {neighbours!r}")
    need = _need(_lib.load(), "dnmf_summary_images_workspace", _int3(sz), NEIGHBOURS[neighbours], int(B), int(segment))
    return _workspace(None, need, device)


def summary_images(frames, sz, sub=None, frame_ids=None, neighbours='full', state=None, first=True, finish=True, segment=0):
    """K18.  frames (rows, ld >= X Y Z) fp32 CUDA rows -> ``(images, state)``: the summary images of the frames seen since
    the state was reset -- ``images`` a dict ``mean / std / max / corr`` of float64 CUDA tensors (X, Y, Z) (None with
    ``finish=False``): per voxel the mean, the population std and the max over time, and the local correlation image, the
    mean Pearson correlation with the ``neighbours`` ('face': 6, 'full': 26; 4 / 8 at Z = 1) that exist, are finite in
    every frame and have a variance > 0 (NaN without one; a voxel with a sample that is not finite is NaN in all four).
    ``sub`` (B, ld >= X Y Z) fp32 CUDA rows: the images of ``frames - sub`` (row j of ``sub`` for the j-th frame of the call),
    bit for bit those of the subtracted rows.  ``frame_ids``: the rows of ``frames`` to take (None: all, in order).  A movie
    larger than one buffer goes in several calls: ``first=True`` resets ``state`` (None: a new one), later calls pass the
    returned ``state`` with ``first=False``, the last one ``finish=True``; a later call may not be larger than the first.
    One pass, float64 sums, no atomics: the same input gives the same bits.  ``segment``: frames per workgroup (0: the
    kernel's choice)."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    if neighbours not in NEIGHBOURS:
        raise ValueError(f"summary_images: neighbours must be 'face' or 'full', got {neighbours!r}")
    fid, B = _frame_rows("summary_images", frames, sub, frame_ids, P)
    dev = frames.device
    lib = _lib.load()
    need = _need(lib, "dnmf_summary_images_workspace", _int3((X, Y, Z)), NEIGHBOURS[neighbours], B, int(segment))
    state = _stream_state("summary_images", state, need, first, dev)
    images = torch.empty((4, X, Y, Z), dtype=torch.float64, device=dev) if finish else None
    with _timed("summary_images"):
        rc = lib.dnmf_summary_images(frames.data_ptr(), _ld(frames, P), _ptr(sub), 0 if sub is None else _ld(sub, P), _ptr(fid),
                                     _int3((X, Y, Z)), B, NEIGHBOURS[neighbours], 1 if first else 0, 1 if finish else 0, int(segment),
                                     state.data_ptr(), _nbytes(state), _ptr(images), _stream())
    _lib.check(rc, "dnmf_summary_images")
    if not finish:
        return None, state
    return dict(mean=images[0], std=images[1], max=images[2], corr=images[3]), state


SELECT_SOURCES = {"value": 0, "absdev": 1, "absdiff": 2}   # DNMF_SELECT_* of include/dnmf_hip.h
TEMPORAL_MAX_QUANTILES = 4


def temporal_quantiles_passes():
    """How often ``temporal_quantiles`` has to see the whole movie: a movie fed in pieces is fed this many times."""
    return _lib.load().dnmf_temporal_select_passes()


class TemporalSelectState:
    """What ``temporal_quantiles`` keeps between the pieces and the passes of one selection: ``buffer``, the device state of
    K30 (``dnmf_temporal_select_workspace``: (8 + 76 Q) bytes a voxel, whatever the number of frames), the arguments the
    selection was started with, ``pass_index``, ``rows`` (fed in this pass so far) and ``rows_per_pass`` (of pass 0, None while
    that one runs)."""

    def __init__(self, buffer, sz, q, source):
        self.buffer, self.sz, self.q, self.source = buffer, tuple(sz), tuple(q), source
        self.pass_index, self.rows, self.rows_per_pass = 0, 0, None


def _interpolated_quantiles(lo, hi, n, q):
    """numpy's ``method='linear'`` in float64 on the two order statistics: the line a_lo + (h - lo)(a_hi - a_lo), h = q (n - 1),
    evaluated from the upper end where h - lo >= 0.5, as numpy does -- (Q, X, Y, Z) float64, NaN where n = 0."""
    qv = torch.tensor(q, dtype=torch.float64, device=lo.device).reshape(-1, 1, 1, 1)
    h = qv * (n.double() - 1.0)[None]
    t = h - torch.floor(h)
    a, b = lo.double(), hi.double()
    d = b - a
    return torch.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def temporal_quantiles(frames, sz, q, source='value', centre=None, frame_ids=None, state=None, first=True, finish=True, segment=0):
    """K30.  frames (rows, ld >= X Y Z) fp32 CUDA rows -> ``(result, state)``: per voxel the exact quantiles ``q`` (1 to 4
    numbers in [0, 1], one call shares every pass over the movie among them) over time of

    * ``source='value'``: the samples themselves;
    * ``'absdev'``: ``|y - centre|`` with ``centre`` an fp32 image of X Y Z voxels (one fp32 subtraction);
    * ``'absdiff'``: ``|y_{t+1} - y_t|`` in the order of the rows (``frame_ids`` order), one term fewer than rows.

    Samples that are not finite are left out.  ``result`` is a dict of CUDA tensors: ``n`` (X, Y, Z) int32, the samples kept;
    ``lo`` and ``hi`` (Q, X, Y, Z) fp32, the kept samples of ranks floor(h) and min(floor(h) + 1, n - 1), h = q (n - 1) --
    input samples, bit for bit (-0 comes back as +0), NaN where n = 0; ``value`` (Q, X, Y, Z) float64, the two interpolated
    like ``np.nanquantile(method='linear')``.  ``frame_ids``: the rows of ``frames`` to take (None: all, in order).

    The selection sees the movie ``temporal_quantiles_passes()`` = 9 times.  With ``first=True, finish=True`` the rows are the
    whole movie and one call does it all.  A movie larger than one buffer goes in pieces, once per pass: the first piece of
    pass 0 has ``first=True`` (``state``: None for a new one, or one to reuse), every later call passes the returned state with
    ``first=False``, and the last piece of each pass has ``finish=True``; ``result`` is None until the last piece of the last
    pass.  Every pass must bring the same rows in the same order, cut in any way: the state counts them, and a pass that
    brings more or fewer rows than pass 0 is refused.  Integer counts only: the same bits on every run and however the movie
    is cut.  State: (8 + 76 Q) bytes a voxel (80 MiB for 512 x 512 x 2 and two quantiles).  ``segment``: frames per workgroup
    (0: the kernel's choice)."""
    fn = "temporal_quantiles"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    qs = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64)).ravel()]
    if not 1 <= len(qs) <= TEMPORAL_MAX_QUANTILES:
        raise ValueError(f"{fn}: {len(qs)} quantiles, 1 to {TEMPORAL_MAX_QUANTILES} a call")
    if not all(0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"{fn}: q must lie in [0, 1], got {qs}")
    if source not in SELECT_SOURCES:
        raise ValueError(f"{fn}: source must be 'value', 'absdev' or 'absdiff', got {source!r}")
    fid, B = _frame_rows(fn, frames, None, frame_ids, P)
    if B < 1:
        raise ValueError(f"{fn}: no rows")
    if fid is not None and (int(fid.min()) < 0 or int(fid.max()) >= frames.shape[0]):
        raise ValueError(f"{fn}: frame_ids must be row indices in [0, {frames.shape[0]})")
    dev = frames.device
    if source == "absdev":
        if centre is None:
            raise ValueError(f"{fn}: source='absdev' needs centre, an fp32 image of {P} voxels")
        if not (isinstance(centre, torch.Tensor) and centre.is_cuda and centre.dtype == torch.float32 and centre.numel() == P
                and centre.is_contiguous()):
            raise ValueError(f"{fn}: centre must be a contiguous float32 CUDA image of {P} voxels")
    else:
        centre = None
    lib = _lib.load()
    need = _need(lib, "dnmf_temporal_select_workspace", _int3((X, Y, Z)), len(qs))
    if first:
        buf = state.buffer if isinstance(state, TemporalSelectState) else None
        state = TemporalSelectState(_workspace(buf, need, dev), (X, Y, Z), qs, source)
    else:
        if not isinstance(state, TemporalSelectState):
            raise ValueError(f"{fn}: first=False needs the state of the earlier calls")
        if (state.sz, state.q, state.source) != ((X, Y, Z), tuple(qs), source):
            raise ValueError(f"{fn}: the selection was started with sz={state.sz}, q={state.q}, source={state.source!r}")
    npass = lib.dnmf_temporal_select_passes()
    if state.pass_index >= npass:
        raise ValueError(f"{fn}: the selection is finished; start another with first=True")
    whole = first and finish
    if state.rows_per_pass is not None and state.rows + B > state.rows_per_pass:
        raise ValueError(f"{fn}: pass {state.pass_index} brings {state.rows + B} rows so far, pass 0 had {state.rows_per_pass}: "
                         f"every pass must bring the same rows")
    if finish and state.rows_per_pass is not None and state.rows + B != state.rows_per_pass:
        raise ValueError(f"{fn}: pass {state.pass_index} ends after {state.rows + B} rows, pass 0 had {state.rows_per_pass}: "
                         f"every pass must bring the same rows")
    qarr = (ctypes.c_double * len(qs))(*qs)
    with _timed(fn):
        for p in (range(npass) if whole else [state.pass_index]):
            rc = lib.dnmf_temporal_select_pass(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3((X, Y, Z)), B, SELECT_SOURCES[source],
                                               _ptr(centre), qarr, len(qs), p, 0 if whole else state.rows, int(segment),
                                               state.buffer.data_ptr(), _nbytes(state.buffer), _stream())
            _lib.check(rc, "dnmf_temporal_select_pass")
    if whole:
        state.pass_index, state.rows, state.rows_per_pass = npass, 0, B
    else:
        state.rows += B
        if finish:
            state.rows_per_pass = state.rows
            state.pass_index, state.rows = state.pass_index + 1, 0
    if state.pass_index < npass:
        return None, state
    Q = len(qs)
    lo = torch.empty((Q, X, Y, Z), dtype=torch.float32, device=dev)
    hi = torch.empty((Q, X, Y, Z), dtype=torch.float32, device=dev)
    n = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    rc = lib.dnmf_temporal_select_finish(_int3((X, Y, Z)), Q, state.buffer.data_ptr(), _nbytes(state.buffer), lo.data_ptr(), hi.data_ptr(),
                                         n.data_ptr(), _stream())
    _lib.check(rc, "dnmf_temporal_select_finish")
    return dict(lo=lo, hi=hi, n=n, value=_interpolated_quantiles(lo, hi, n, qs)), state


NOISE_DIFF_SCALE = 1.4826 / math.sqrt(2.0)   # K21's estimate of a trace's noise from its adjacent differences (deconvolve_traces)
NOISE_MAD_SCALE = 1.4826


def _quantiles_of_pieces(pieces, sz, q, source='value', centre=None):
    """``temporal_quantiles`` of a movie that ``pieces()`` serves as an iterable of row tensors, once per pass."""
    state = result = None
    for p in range(temporal_quantiles_passes()):
        prev = None
        for rows in pieces():
            if prev is not None:
                _, state = temporal_quantiles(prev, sz, q, source, centre, state=state, first=p == 0 and state is None, finish=False)
            prev = rows
        if prev is None:
            raise ValueError("robust_images: no frames")
        result, state = temporal_quantiles(prev, sz, q, source, centre, state=state, first=p == 0 and state is None, finish=True)
        if result is not None:       # the last pass, or a movie of one piece, which one call takes through every pass
            return result


def robust_images(pieces, sz, percentiles=(), noise='diff'):
    """The order-statistic images of a movie (K30, ``temporal_quantiles``; tests/robust_restatement.py R6): a dict of float64
    CUDA images (X, Y, Z) -- ``median``, ``max``, ``mad`` = median |y - fp32(median)|, ``noise`` ('diff': median |y_{t+1} - y_t|
    x 1.4826 / sqrt(2), the constants of the estimate ``deconvolve_traces`` makes per trace; 'mad': 1.4826 mad),
    ``pnr`` = (max - median) / noise (NaN where noise is 0 or not finite, or n < 2), ``n`` int32 (the finite samples) and
    ``percentile`` {p: image} for every p of ``percentiles`` (in [0, 100]).  ``pieces``: fp32 CUDA rows (T, ld >= X Y Z), or
    a callable that returns an iterable of such pieces, in the same order at every call -- it is called once per pass, 9
    passes for every selection: one for median, max and the first two percentiles, one per further four percentiles, one
    for mad and, with noise='diff', one for the noise."""
    if noise not in ("diff", "mad"):
        raise ValueError(f"robust_images: noise must be 'diff' or 'mad', got {noise!r}")
    ps = list(percentiles)
    if not all(0.0 <= float(p) <= 100.0 for p in ps):
        raise ValueError(f"robust_images: percentiles must lie in [0, 100], got {ps}")
    if isinstance(pieces, torch.Tensor):
        rows = pieces
        pieces = lambda: (rows,)     # noqa: E731
    qs = [0.5, 1.0] + [float(p) / 100.0 for p in ps]
    values, n = [], None
    for s in range(0, len(qs), TEMPORAL_MAX_QUANTILES):
        r = _quantiles_of_pieces(pieces, sz, qs[s:s + TEMPORAL_MAX_QUANTILES])
        values.extend(r["value"])
        n = r["n"] if n is None else n
    median, mx = values[0], values[1]
    mad = _quantiles_of_pieces(pieces, sz, [0.5], 'absdev', median.float().contiguous())["value"][0]
    if noise == "diff":
        sigma = _quantiles_of_pieces(pieces, sz, [0.5], 'absdiff')["value"][0] * NOISE_DIFF_SCALE
    else:
        sigma = NOISE_MAD_SCALE * mad
    ok = torch.isfinite(sigma) & (sigma != 0) & (n >= 2)
    pnr = torch.where(ok, (mx - median) / sigma, torch.full_like(sigma, float("nan")))
    return dict(median=median, max=mx, mad=mad, noise=sigma, pnr=pnr, n=n, percentile={p: values[2 + i] for i, p in enumerate(ps)})


def noise_image(pieces, sz):
    """The ``noise`` image of ``robust_images(noise='diff')`` alone (one selection, 9 passes): float64 CUDA (X, Y, Z)."""
    if isinstance(pieces, torch.Tensor):
        rows = pieces
        pieces = lambda: (rows,)     # noqa: E731
    return _quantiles_of_pieces(pieces, sz, [0.5], 'absdiff')["value"][0] * NOISE_DIFF_SCALE


RUNNING_MAX_WINDOW = 2048                                                # a window of K31a lives in LDS
BASELINE_MODES = {"baseline": 0, "df": 1, "dff": 2, "dfsqrtf": 3}        # DNMF_BASELINE_* of include/dnmf_hip.h


def _window_args(fn, window, stride):
    if int(window) != window or int(window) < 1:
        raise ValueError(f"{fn}: window={window!r}: a number of frames, at least 1")
    window = int(window)
    if window > RUNNING_MAX_WINDOW:
        raise ValueError(f"{fn}: window={window} frames, at most {RUNNING_MAX_WINDOW} (a window lives in LDS; nothing is truncated)")
    stride = max(1, window // 4) if stride is None else stride
    if int(stride) != stride or not 1 <= int(stride) <= window:
        raise ValueError(f"{fn}: stride={stride!r} outside [1, window={window}]")
    return window, int(stride)


def running_window_plan(T, window, stride=None):
    """The windows K31 covers a movie of ``T`` frames with (tests/dff_restatement.py D1; host only, integers, the plan the kernel
    uses): a dict ``J``, ``starts`` and ``ends`` (J,) int64 -- window j holds the frames [starts[j], ends[j]), starts[j] =
    min(j stride, max(T - window, 0)), the last one ends at T -- and ``centres`` (J,) float64, (start + end - 1) / 2, where the
    knots sit.  ``stride=None``: max(1, window // 4)."""
    fn = "running_window_plan"
    window, stride = _window_args(fn, window, stride)
    if int(T) != T or int(T) < 1:
        raise ValueError(f"{fn}: T={T!r} frames")
    T = int(T)
    J = 1 if T <= window else -((window - T) // stride) + 1
    starts = np.minimum(np.arange(J, dtype=np.int64) * stride, max(T - window, 0))
    ends = np.minimum(starts + window, T)
    return dict(J=J, starts=starts, ends=ends, centres=(starts + ends - 1).astype(np.float64) / 2.0)


def running_quantile(frames, sz, window, stride=None, q=0.08, frame_ids=None, min_samples=1, row0=0, T=None, run=0):
    """K31a.  frames (rows, ld >= X Y Z) fp32 CUDA rows in time order -> per voxel the exact quantile ``q`` in [0, 1] of every
    window of ``window`` frames, one every ``stride`` frames (None: max(1, window // 4)), of ``running_window_plan``: a dict of

    * ``n`` (J, X, Y, Z) int32, the finite samples of the window (the others are left out, as in ``temporal_quantiles``);
    * ``lo``, ``hi`` (J, X, Y, Z) fp32, the kept samples of ranks floor(h) and min(floor(h) + 1, n - 1), h = q (n - 1): input
      samples, bit for bit (-0 comes back as +0), NaN where n = 0;
    * ``value`` (J, X, Y, Z) float64, the two interpolated like ``np.nanquantile(method='linear')``, NaN where n < ``min_samples``;
    * ``centres``, ``starts``, ``ends`` of the plan, and ``windows = (j0, j1)``.

    The rows are the frames ``row0 .. row0 + rows - 1`` of a movie of ``T`` frames (None: the rows are the movie), taken in the
    order of ``frame_ids`` where given.  Computed are exactly the windows j0 .. j1 - 1 that lie wholly inside the rows; the
    others are NaN / 0 in the tables.  A movie that goes in pieces overlaps them by up to window - stride rows so that every
    window is whole in some piece; the tables of the pieces, put together, equal those of one call bit for bit.  ``run``:
    windows per workgroup (0: the kernel's choice); the result does not depend on it.  No workspace, integer counts only."""
    fn = "running_quantile"
    window, stride = _window_args(fn, window, stride)
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"{fn}: q must lie in [0, 1], got {q}")
    if int(min_samples) < 1:
        raise ValueError(f"{fn}: min_samples={min_samples!r}, at least 1")
    if int(run) < 0:
        raise ValueError(f"{fn}: run={run!r}: windows per workgroup, 0 for the kernel's choice")
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows(fn, frames, None, frame_ids, P)
    if B < 1:
        raise ValueError(f"{fn}: no rows")
    if fid is not None and (int(fid.min()) < 0 or int(fid.max()) >= frames.shape[0]):
        raise ValueError(f"{fn}: frame_ids must be row indices in [0, {frames.shape[0]})")
    row0 = int(row0)
    T = row0 + B if T is None else int(T)
    if row0 < 0 or row0 + B > T:
        raise ValueError(f"{fn}: rows {row0} .. {row0 + B} of a movie of T={T} frames")
    plan = running_window_plan(T, window, stride)
    J, dev = plan["J"], frames.device
    lo = torch.full((J, X, Y, Z), float("nan"), dtype=torch.float32, device=dev)
    hi = torch.full((J, X, Y, Z), float("nan"), dtype=torch.float32, device=dev)
    n = torch.zeros((J, X, Y, Z), dtype=torch.int32, device=dev)
    lib = _lib.load()
    win = (ctypes.c_long * 2)()
    with _timed(fn):
        rc = lib.dnmf_running_quantile(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3((X, Y, Z)), B, row0, T, window, stride, q,
                                       int(run), lo.data_ptr(), hi.data_ptr(), n.data_ptr(), P, win, _stream())
    _lib.check(rc, "dnmf_running_quantile")
    value = _interpolated_quantiles(lo, hi, n, [q])[0]
    if int(min_samples) > 1:
        value = torch.where(n >= int(min_samples), value, torch.full_like(value, float("nan")))
    return dict(lo=lo, hi=hi, n=n, value=value, centres=plan["centres"], starts=plan["starts"], ends=plan["ends"],
                windows=(int(win[0]), int(win[1])))


def _overlap(a, b):
    """Whether the storages of two tensors share a byte."""
    sa, sb = a.untyped_storage(), b.untyped_storage()
    return sa.data_ptr() < sb.data_ptr() + sb.nbytes() and sb.data_ptr() < sa.data_ptr() + sa.nbytes()


def baseline_apply(frames, sz, value, centres, mode='dff', offset=0.0, frame_ids=None, row0=0, out=None):
    """K31b.  frames (rows, ld >= X Y Z) fp32 CUDA rows, the frames ``row0 .. row0 + rows - 1`` of the movie (in the order of
    ``frame_ids`` where given), read against the baseline that runs through the knots ``value`` (J, X, Y, Z) float64 at the
    frames ``centres`` (J,), strictly increasing -- what ``running_quantile`` returned: F0 is the first knot before the first
    centre, the last one after the last, and between two centres their line, in float64 (tests/dff_restatement.py D3).
    -> (rows, P) fp32 by ``mode``: ``'baseline'`` F0, ``'df'`` y - F0, ``'dff'`` (y - F0) / (F0 + offset), ``'dfsqrtf'``
    (y - F0) / sqrt(F0 + offset), computed in float64 and rounded once; NaN where y or F0 is not finite and, in the last two,
    where F0 + offset <= 0.  ``out``: rows to write (None: new ones); it may not share memory with ``frames``.  One streaming
    launch."""
    fn = "baseline_apply"
    if mode not in BASELINE_MODES:
        raise ValueError(f"{fn}: mode must be one of {sorted(BASELINE_MODES)}, got {mode!r}")
    offset = float(offset)
    if not math.isfinite(offset):
        raise ValueError(f"{fn}: offset={offset} is not finite")
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows(fn, frames, None, frame_ids, P)
    if B < 1:
        raise ValueError(f"{fn}: no rows")
    if fid is not None and (int(fid.min()) < 0 or int(fid.max()) >= frames.shape[0]):
        raise ValueError(f"{fn}: frame_ids must be row indices in [0, {frames.shape[0]})")
    dev = frames.device
    c = torch.from_numpy(np.array(centres.cpu() if isinstance(centres, torch.Tensor) else centres, dtype=np.float64).ravel())
    J = c.numel()
    if J < 1 or not bool((c[1:] > c[:-1]).all()) or not bool(torch.isfinite(c).all()):
        raise ValueError(f"{fn}: centres must be at least one finite frame position, strictly increasing")
    if not (isinstance(value, torch.Tensor) and value.is_cuda and value.dtype == torch.float64 and value.is_contiguous()
            and value.numel() == J * P):
        raise ValueError(f"{fn}: value must be a contiguous float64 CUDA tensor of {J} knots x {P} voxels")
    if int(row0) < 0:
        raise ValueError(f"{fn}: row0={row0!r}")
    if out is not None and isinstance(out, torch.Tensor) and _overlap(out, frames):
        raise ValueError(f"{fn}: out may not share memory with frames")
    out = _out_rows(fn, out, B, P, dev)
    lib, cdev = _lib.load(), c.to(dev)
    with _timed(fn):
        rc = lib.dnmf_baseline_apply(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3((X, Y, Z)), B, int(row0), value.data_ptr(), P,
                                     cdev.data_ptr(), J, BASELINE_MODES[mode], offset, out.data_ptr(), _ld(out, P), _stream())
    _lib.check(rc, "dnmf_baseline_apply")
    return out[:B, :P]


def _running_pieces(T, P, window, stride, limit=None):
    """How a movie of ``T`` frames goes through K31 in pieces of at most 1 GiB (``limit`` rows; at least one window): a list of
    ``(r0, r1, j0, j1)`` -- the rows [r0, r1) hold exactly the windows j0 .. j1 - 1 whole, consecutive pieces overlap by up to
    window - stride rows, and every window is in one piece."""
    plan = running_window_plan(T, window, stride)
    starts, ends, J = plan["starts"], plan["ends"], plan["J"]
    limit = max(int(ends[0] - starts[0]), (1 << 30) // (4 * P) if limit is None else int(limit))
    pieces, j0 = [], 0
    while j0 < J:
        j1 = j0 + 1
        while j1 < J and ends[j1] - starts[j0] <= limit:
            j1 += 1
        pieces.append((int(starts[j0]), int(ends[j1 - 1]), j0, j1))
        j0 = j1
    return plan, pieces


def dff_rows(rows_of, T, sz, window, stride=None, q=0.08, mode='dff', offset=0.0, min_samples=1, limit=None, out=None):
    """K31a then K31b on a movie of ``T`` frames that ``rows_of(r0, r1)`` serves as fp32 CUDA rows (r1 - r0, ld >= P) in time
    order, in pieces of at most 1 GiB (``limit``: rows a piece, for tests) -> ``(movie (T, P) fp32 CUDA, info)`` with
    ``info = dict(knots (J, X, Y, Z) float64, centres, n, starts, ends)``: the same bits however the movie is cut."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    window, stride = _window_args("dff_rows", window, stride)
    plan, pieces = _running_pieces(T, P, window, stride, limit)
    knots = n = None
    for r0, r1, j0, j1 in pieces:
        r = running_quantile(rows_of(r0, r1), sz, window, stride, q, min_samples=min_samples, row0=r0, T=T)
        got0, got1 = r["windows"]
        assert got0 <= j0 and j1 <= got1, (r["windows"], j0, j1)
        if knots is None:
            knots, n = r["value"], r["n"]
        else:
            knots[j0:j1], n[j0:j1] = r["value"][j0:j1], r["n"][j0:j1]
    dev = knots.device
    movie = _out_rows("dff_rows", out, T, P, dev)
    step = max(1, min(T, (1 << 30) // (4 * P) if limit is None else int(limit)))
    for r0 in range(0, T, step):
        r1 = min(T, r0 + step)
        baseline_apply(rows_of(r0, r1), sz, knots, plan["centres"], mode, offset, row0=r0, out=movie[r0:r1])
    return movie[:T, :P], dict(knots=knots, centres=plan["centres"], n=n, starts=plan["starts"], ends=plan["ends"])


LOWRANK_MAX_VOXELS = 1024      # a patch of K34 lives in LDS (csrc/lowrank_denoise.hip: LR_MAX_VOXELS)
LOWRANK_MAX_RANK = 8
LOWRANK_SWEEPS = 10            # the Jacobi sweeps of K34d: a parameter of the algorithm, not a tolerance


def lowrank_patch_plan(sz, patch=(16, 16, None), overlap=(8, 8, 0)):
    """The patches K34 covers a volume with (tests/denoise_restatement.py L1; host only, integers): along each axis the stride is
    patch - overlap, patch i starts at min(i stride, max(extent - patch, 0)) -- the clamp of ``running_window_plan`` -- and the last
    one ends at the extent; a patch larger than the axis is the axis; ``None`` in z is min(Z, 4).  Every patch has the same
    ``shape``; ``n``, its voxels, is at most 1024 (ValueError beyond: a patch is never cut).  -> a dict ``boxes`` (NP, 6) int32
    inclusive [x0, x1, y0, y1, z0, z1], x slowest as K24's, ``counts``, ``shape``, ``strides`` per axis, ``starts`` and ``n``."""
    fn = "lowrank_patch_plan"
    sz = [int(s) for s in sz]
    if len(sz) != 3 or min(sz) < 1 or len(patch) != 3 or len(overlap) != 3:
        raise ValueError(f"{fn}: sz={sz}, patch={patch!r}, overlap={overlap!r}: three axes, extents of at least 1")
    patch = [patch[0], patch[1], min(sz[2], 4) if patch[2] is None else patch[2]]
    starts, lens, strides = [], [], []
    for a, (ext, pa, ov) in enumerate(zip(sz, patch, overlap)):
        if int(pa) != pa or int(ov) != ov or int(pa) < 1 or not 0 <= int(ov) < int(pa):
            raise ValueError(f"{fn}: axis {a}: patch={pa!r}, overlap={ov!r}: whole numbers with 0 <= overlap < patch")
        pa, ov = int(pa), int(ov)
        stride = pa - ov
        count = 1 if ext <= pa else -((pa - ext) // stride) + 1
        starts.append(np.minimum(np.arange(count, dtype=np.int64) * stride, max(ext - pa, 0)))
        lens.append(min(pa, ext))
        strides.append(stride)
    n = lens[0] * lens[1] * lens[2]
    if n > LOWRANK_MAX_VOXELS:
        raise ValueError(f"{fn}: a patch of {lens[0]}x{lens[1]}x{lens[2]} = {n} voxels, at most {LOWRANK_MAX_VOXELS} (a patch lives "
                         f"in LDS; it is never cut)")
    sx, sy, s_z = np.meshgrid(*starts, indexing="ij")
    lo = np.stack([sx.ravel(), sy.ravel(), s_z.ravel()], 1)
    boxes = np.empty((lo.shape[0], 6), dtype=np.int32)
    boxes[:, 0::2], boxes[:, 1::2] = lo, lo + np.array(lens) - 1
    return dict(boxes=boxes, counts=tuple(len(s) for s in starts), shape=tuple(lens), strides=tuple(strides), starts=tuple(starts),
                n=n, sz=tuple(sz))


def _lowrank_plan(plan):
    """(the 9 ints of the C ABI, NP, n) of a ``lowrank_patch_plan``."""
    ints = [v for a in range(3) for v in (plan["counts"][a], plan["strides"][a], plan["shape"][a])]
    return (ctypes.c_int * 9)(*ints), len(plan["boxes"]), plan["n"]


def _lowrank_image(fn, name, img, P, dev):
    if img is None:
        return None
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.numel() != P:
        raise ValueError(f"{fn}: {name} must be an (X, Y, Z) image of {P} voxels, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float64).contiguous()


def _lowrank_rank(fn, rank):
    if int(rank) != rank or not 1 <= int(rank) <= LOWRANK_MAX_RANK:
        raise ValueError(f"{fn}: rank={rank!r} outside [1, {LOWRANK_MAX_RANK}]")
    return int(rank)


def lowrank_state(plan, rank, T, device="cuda"):
    """The state of K34 for the patches of ``plan``, ``rank`` = R columns and a movie of ``T`` frames, float64 on the device: ``U``,
    ``W`` (NP, n, R), ``Q`` (NP, T, R), ``energy`` (NP, T), ``lam`` (NP, R), ``explained`` (NP,), and ``kept``, ``ok`` (NP,) int32
    (ok = 1).  U is the orthonormalised start U0[v, j] = cos(pi (v + 1/2) j / n) (K34b on the host's table), W is zero."""
    fn = "lowrank_state"
    R = _lowrank_rank(fn, rank)
    if int(T) != T or int(T) < 1:
        raise ValueError(f"{fn}: T={T!r} frames")
    _, NP, n = _lowrank_plan(plan)
    f64 = dict(dtype=torch.float64, device=device)
    v = np.arange(n, dtype=np.float64)[:, None]
    u0 = torch.from_numpy(np.cos(np.pi * (v + 0.5) * np.arange(R, dtype=np.float64)[None, :] / n)).to(device)
    state = dict(plan=plan, rank=R, T=int(T), U=torch.zeros((NP, n, R), **f64), W=u0[None].repeat(NP, 1, 1).contiguous(),
                 Q=torch.zeros((NP, int(T), R), **f64), energy=torch.zeros((NP, int(T)), **f64), lam=torch.zeros((NP, R), **f64),
                 explained=torch.zeros((NP,), **f64), kept=torch.zeros((NP,), dtype=torch.int32, device=device),
                 ok=torch.ones((NP,), dtype=torch.int32, device=device))
    return lowrank_orthonormalise(state)


def _lowrank_call(fn, frames, sz, plan, state, centre, scale, frame_ids, row0):
    """The checks every pass of K34 over frames shares -> (fid, B, P, plan ints, centre, scale)."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    if tuple(plan["sz"]) != (X, Y, Z) or state["plan"] is not plan and state["plan"]["boxes"].shape != plan["boxes"].shape:
        raise ValueError(f"{fn}: the plan is one of a volume {plan['sz']}, the state one of {state['plan']['sz']}, sz={(X, Y, Z)}")
    fid, B = _frame_rows(fn, frames, None, frame_ids, P)
    if B < 1:
        raise ValueError(f"{fn}: no rows")
    if fid is not None and (int(fid.min()) < 0 or int(fid.max()) >= frames.shape[0]):
        raise ValueError(f"{fn}: frame_ids must be row indices in [0, {frames.shape[0]})")
    if int(row0) < 0 or int(row0) + B > state["T"]:
        raise ValueError(f"{fn}: rows {row0} .. {int(row0) + B} of a movie of T={state['T']} frames")
    dev = frames.device
    c = _lowrank_image(fn, "centre", centre, P, dev)
    if c is None:
        raise ValueError(f"{fn}: centre is required (scale=None means ones)")
    return fid, B, P, _lowrank_plan(plan)[0], c, _lowrank_image(fn, "scale", scale, P, dev)


def lowrank_accumulate(frames, sz, plan, state, centre, scale=None, frame_ids=None, row0=0):
    """K34a.  ``state['W'] += D (D^T U)`` per patch over the fp32 CUDA rows ``frames`` (rows, ld >= X Y Z), the frames ``row0 ..``
    of the movie: one pass over the movie per subspace iteration, in as many calls as the movie has pieces -- the same bits
    however it is cut.  D = (y - centre) / scale with float64 (X, Y, Z) images (``scale=None``: ones).  Clears ``state['ok']`` of a
    patch with a sample or centre that is not finite, or a scale that is not finite or <= 0.  -> state."""
    fn = "lowrank_accumulate"
    fid, B, P, plan9, c, s = _lowrank_call(fn, frames, sz, plan, state, centre, scale, frame_ids, row0)
    with _timed(fn):
        rc = _lib.load().dnmf_lowrank_accumulate(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3(sz), B, plan9, state["rank"],
                                                 c.data_ptr(), _ptr(s), state["U"].data_ptr(), state["W"].data_ptr(),
                                                 state["ok"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_lowrank_accumulate")
    return state


def lowrank_orthonormalise(state):
    """K34b.  ``U = MGS(W)`` per patch, in column order (a column whose norm after the projections is <= 1e-12 x its norm before
    becomes zero), and ``W = 0``; U = 0 where ok = 0.  -> state."""
    _, NP, n = _lowrank_plan(state["plan"])
    with _timed("lowrank_orthonormalise"):
        rc = _lib.load().dnmf_lowrank_orthonormalise(NP, n, state["rank"], state["U"].data_ptr(), state["W"].data_ptr(),
                                                     state["ok"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_lowrank_orthonormalise")
    return state


def lowrank_project(frames, sz, plan, state, centre, scale=None, frame_ids=None, row0=0):
    """K34c.  Rows ``row0 ..`` of ``state['Q']`` = D^T U and of ``state['energy']`` = sum_v D^2, for the rows given.  -> state."""
    fn = "lowrank_project"
    fid, B, P, plan9, c, s = _lowrank_call(fn, frames, sz, plan, state, centre, scale, frame_ids, row0)
    with _timed(fn):
        rc = _lib.load().dnmf_lowrank_project(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3(sz), B, int(row0), state["T"], plan9,
                                              state["rank"], c.data_ptr(), _ptr(s), state["U"].data_ptr(), state["Q"].data_ptr(),
                                              state["energy"].data_ptr(), state["ok"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_lowrank_project")
    return state


def lowrank_edge(n, T, threshold=1.0):
    """(threshold (sqrt n + sqrt T))^2: the Marchenko-Pastur edge of the largest eigenvalue of N^T N for n x T unit noise."""
    return (float(threshold) * (math.sqrt(float(n)) + math.sqrt(float(T)))) ** 2


def lowrank_ritz(state, keep='auto', threshold=1.0, n=None, T=None, sweeps=LOWRANK_SWEEPS):
    """K34d.  Per patch B = Q^T Q, ``sweeps`` sweeps of cyclic Jacobi, ``lam`` descending (ties by index), U and Q rotated to match;
    ``kept``: ``keep='auto'`` the number of lam > (threshold (sqrt n + sqrt T))^2, ``keep=r`` the number of lam > 0 among the first r;
    ``explained`` = the kept lam over sum D^2.  ``n``, ``T``: those of the edge (None: the state's).  -> state."""
    fn = "lowrank_ritz"
    _, NP, pn = _lowrank_plan(state["plan"])
    n, T = pn if n is None else int(n), state["T"] if T is None else int(T)
    threshold = float(threshold)
    if keep == 'auto':
        if not (math.isfinite(threshold) and threshold >= 0.0):
            raise ValueError(f"{fn}: threshold={threshold!r}: a finite factor >= 0")
        k, e = -1, lowrank_edge(n, T, threshold)
    else:
        if isinstance(keep, str) or int(keep) != keep or int(keep) < 0:
            raise ValueError(f"{fn}: keep must be 'auto' or a number of columns >= 0, got {keep!r}")
        k, e = min(int(keep), state["rank"]), 0.0
    if int(sweeps) != sweeps or not 0 <= int(sweeps) <= 64:
        raise ValueError(f"{fn}: sweeps={sweeps!r} outside [0, 64]")
    with _timed(fn):
        rc = _lib.load().dnmf_lowrank_ritz(NP, pn, state["T"], state["rank"], k, e, int(sweeps), state["U"].data_ptr(),
                                           state["Q"].data_ptr(), state["energy"].data_ptr(), state["ok"].data_ptr(),
                                           state["lam"].data_ptr(), state["kept"].data_ptr(), state["explained"].data_ptr(), _stream())
    _lib.check(rc, "dnmf_lowrank_ritz")
    return state


def lowrank_reconstruct(frames, sz, plan, state, centre, scale=None, frame_ids=None, row0=0, out=None):
    """K34e.  The blended movie of the rows ``row0 ..``: per voxel the tent-weighted mean, over the ok patches that hold it, of
    centre + scale sum_{j < kept} U[v, j] Q[t, j], float64 rounded once -> (rows, P) fp32.  ``frames`` is read only where no ok patch
    holds the voxel: those samples come back bit for bit."""
    fn = "lowrank_reconstruct"
    fid, B, P, plan9, c, s = _lowrank_call(fn, frames, sz, plan, state, centre, scale, frame_ids, row0)
    out = _out_rows(fn, out, B, P, frames.device)
    with _timed(fn):
        rc = _lib.load().dnmf_lowrank_reconstruct(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3(sz), B, int(row0), state["T"], plan9,
                                                  state["rank"], c.data_ptr(), _ptr(s), state["U"].data_ptr(), state["Q"].data_ptr(),
                                                  state["kept"].data_ptr(), state["ok"].data_ptr(), out.data_ptr(), _ld(out, P),
                                                  _stream())
    _lib.check(rc, "dnmf_lowrank_reconstruct")
    return out[:B, :P]


def lowrank_denoise(frames, sz, centre, scale=None, patch=(16, 16, None), overlap=(8, 8, 0), rank=8, keep='auto', threshold=1.0, iters=4,
                    sweeps=LOWRANK_SWEEPS, T=None, limit=None, out=None):
    """K34 (tests/denoise_restatement.py): the movie denoised by local low-rank approximation -> ``(out (T, P) fp32 CUDA, info)``.
    ``frames``: fp32 CUDA rows (T, ld >= X Y Z) of a registered movie, or a callable ``rows_of(r0, r1)`` that serves the rows
    [r0, r1) of a movie of ``T`` frames; it goes through in pieces of at most 1 GiB (``limit`` rows, for tests), once per pass:
    ``iters`` >= 1 passes of K34a + K34b, one of K34c, K34d, one of K34e.  Per patch of ``lowrank_patch_plan(sz, patch, overlap)``
    the ``rank`` <= 8 leading singular pairs of D = (y - centre) / scale, of which ``keep`` are used ('auto': those above
    ``threshold`` x the noise edge sqrt n + sqrt T of unit noise, which presumes ``scale`` is the noise level).  ``info``: ``plan``,
    ``kept``, ``lam`` (the squared singular values), ``ok``, ``explained`` and the factors ``U`` (NP, n, R), ``Q`` (NP, T, R).
    The same bits on every run and for every ``limit``."""
    fn = "lowrank_denoise"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    if int(iters) != iters or int(iters) < 1:
        raise ValueError(f"{fn}: iters={iters!r}: at least one pass (the first one finds the patches that cannot be used)")
    if isinstance(frames, torch.Tensor):
        rows = frames
        T, rows_of, dev = rows.shape[0], (lambda r0, r1: rows[r0:r1]), rows.device
    else:
        rows_of = frames
        if T is None:
            raise ValueError(f"{fn}: a callable frames needs T")
        dev = rows_of(0, 1).device
    T = int(T)
    plan = lowrank_patch_plan((X, Y, Z), patch, overlap)
    step = max(1, min(T, (1 << 30) // (4 * P) if limit is None else int(limit)))
    state = lowrank_state(plan, rank, T, dev)
    c, s = _lowrank_image(fn, "centre", centre, P, dev), _lowrank_image(fn, "scale", scale, P, dev)

    def pieces():
        for r0 in range(0, T, step):
            yield r0, rows_of(r0, min(T, r0 + step))
    for _ in range(int(iters)):
        for r0, fr in pieces():
            lowrank_accumulate(fr, sz, plan, state, c, s, row0=r0)
        lowrank_orthonormalise(state)
    for r0, fr in pieces():
        lowrank_project(fr, sz, plan, state, c, s, row0=r0)
    lowrank_ritz(state, keep, threshold, sweeps=sweeps)
    movie = _out_rows(fn, out, T, P, dev)
    for r0, fr in pieces():
        lowrank_reconstruct(fr, sz, plan, state, c, s, row0=r0, out=movie[r0:r0 + fr.shape[0]])
    info = dict(plan=plan, kept=state["kept"], lam=state["lam"], ok=state["ok"], explained=state["explained"], U=state["U"],
                Q=state["Q"])
    return movie[:T, :P], info


def _pass_rows(frames, sub, fid, P):
    """What every pass over the movie is given first: frames, ldf, sub, lds, frame_ids as the library takes them."""
    return frames.data_ptr(), _ld(frames, P), _ptr(sub), 0 if sub is None else _ld(sub, P), _ptr(fid)


def _scratch(need, dev):
    """A workspace of ``need`` bytes that nothing outlives the call (float64: 8-byte aligned, as the passes ask)."""
    return torch.empty(((need + 7) // 8,), dtype=torch.float64, device=dev)


def background_state(sz, B, segment=0, device="cuda"):
    """An empty state for ``background_accum`` calls of up to ``B`` frames each; pass it with ``first=True``."""
    X, Y, Z = (int(s) for s in sz)
    return _workspace(None, _need(_lib.load(), "dnmf_background_accum_workspace", X * Y * Z, int(B), int(segment)), device)


def background_dots(frames, b, sub=None, frame_ids=None):
    """K19, the f half-step.  frames (rows, ld >= P) fp32 CUDA rows, ``b`` fp32 CUDA of P voxels (any shape), ``sub`` (B, ld >= P)
    the model's prediction of the frames of the call (None: nothing) -> ``(f, num, bb)``: ``num[j] = sum_p b_p (frames - sub)[j, p]``
    (B float64), ``bb = sum_p b_p^2`` (one float64, on the GPU) and ``f = max(0, num) / bb`` rounded to fp32 (0 when bb == 0), the
    exact minimiser of ``|frames - sub - b f|^2`` over f >= 0.  The difference is taken in float64 as the rows are read; no
    subtracted movie is made.  ``frame_ids``: the rows of ``frames`` to take (None: all, in order).  Float64 sums in a fixed
    order: the same input gives the same bits.  Everything must be finite."""
    b = _f32(b, "b").reshape(-1)
    P = b.numel()
    fid, B = _frame_rows("background_dots", frames, sub, frame_ids, P)
    dev = frames.device
    lib = _lib.load()
    ws = _scratch(_need(lib, "dnmf_background_dots_workspace", P, B), dev)
    num = torch.empty((B,), dtype=torch.float64, device=dev)
    bb = torch.empty((1,), dtype=torch.float64, device=dev)
    f = torch.empty((B,), dtype=torch.float32, device=dev)
    with _timed("background_dots"):
        rc = lib.dnmf_background_dots(*_pass_rows(frames, sub, fid, P), b.data_ptr(), P, B, num.data_ptr(), bb.data_ptr(), f.data_ptr(),
                                      ws.data_ptr(), _nbytes(ws), _stream())
    _lib.check(rc, "dnmf_background_dots")
    return f, num, bb


def background_accum(frames, f, sz, sub=None, frame_ids=None, state=None, first=True, finish=True, segment=0):
    """K19, the b half-step.  frames (rows, ld >= X Y Z) fp32 CUDA rows, ``f`` fp32 CUDA with one value per frame of the call,
    ``sub`` as in ``background_dots`` -> ``((b, num, ff) or None, state)``: over the frames seen since the state was reset
    ``num[p] = sum_t f_t (frames - sub)[t, p]`` ((X, Y, Z) float64), ``ff = sum_t f_t^2`` (one float64, on the GPU) and
    ``b = max(0, num) / ff`` rounded to fp32 ((X, Y, Z); 0 when ff == 0), the exact minimiser over b >= 0.  A movie larger than one
    buffer goes in several calls: ``first=True`` resets ``state`` (None: a new one), later calls pass the returned ``state``
    with ``first=False``, the last one ``finish=True`` (before that the triple is None); a later call may not be larger than
    the first.  The result of several calls is that of one up to the order of the float64 sums.  ``segment``: frames per
    workgroup (0: the kernel's choice).  No atomics: the same input gives the same bits."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows("background_accum", frames, sub, frame_ids, P)
    f = _f32(f, "f").reshape(-1)
    if f.numel() != B:
        raise ValueError(f"background_accum: f must hold one value for each of the {B} frames, got {f.numel()}")
    dev = frames.device
    lib = _lib.load()
    need = _need(lib, "dnmf_background_accum_workspace", P, B, int(segment))
    state = _stream_state("background_accum", state, need, first, dev)
    b =torch.empty((X, Y, Z), dtype=torch.float32, device=dev) if finish else None
    num = torch.empty((X, Y, Z), dtype=torch.float64, device=dev) if finish else None
    ff = torch.empty((1,), dtype=torch.float64, device=dev) if finish else None
    with _timed("background_accum"):
        rc = lib.dnmf_background_accum(*_pass_rows(frames, sub, fid, P), f.data_ptr(), P, B, 1 if first else 0, 1 if finish else 0,
                                       int(segment), state.data_ptr(), _nbytes(state), _ptr(b), _ptr(num), _ptr(ff), _stream())
    _lib.check(rc, "dnmf_background_accum")
    return ((b, num, ff) if finish else None), state


def _subtract_rows(fn, frames, frame_ids, times, P):
    """The checks the two subtractions share -> (frame_ids, times: int32 or None, frames of the call)."""
    _frame_rows(fn, frames, None, None, P)
    fid, tt, B = _ids(frames, frame_ids, times, frames.device)
    if fid is not None and fid.numel() != B:
        raise ValueError(f"{fn}: {fid.numel()} frame_ids for {B} times")
    if fid is None and B > frames.shape[0]:
        raise ValueError(f"{fn}: {B} times for {frames.shape[0]} frames")
    return fid, tt, B


def background_subtract(frames, b, f, frame_ids=None, times=None, out=None, clamp=True):
    """K19.  ``out[j] = frames[row j] - b f[t_j]`` as one fp32 fused multiply-add per voxel, ``max(., 0)`` with ``clamp``: (B, P) fp32
    CUDA rows.  ``frame_ids``: the rows of ``frames`` to take (None: all, in order); ``times``: the entry of ``f`` of each frame of
    the call (None: j; an entry ``f`` does not have makes the row NaN).  ``out=frames`` works in place (``frame_ids`` None).
    ``f`` as (R, T) with ``b`` of R images is the rank-R background of K23: ``background_subtract_rank``."""
    if isinstance(f, torch.Tensor) and f.dim() == 2:
        return background_subtract_rank(frames, b, f, frame_ids=frame_ids, times=times, out=out, clamp=clamp)
    b = _f32(b, "b").reshape(-1)
    f = _f32(f, "f").reshape(-1)
    P = b.numel()
    fid, tt, B = _subtract_rows("background_subtract", frames, frame_ids, times, P)
    out = _out_rows("background_subtract", out, B, P, frames.device)
    lib = _lib.load()
    with _timed("background_subtract"):
        rc = lib.dnmf_background_subtract(frames.data_ptr(), _ld(frames, P), _ptr(fid), b.data_ptr(), f.data_ptr(), f.numel(), _ptr(tt),
                                          P, B, out.data_ptr(), _ld(out, P), 1 if clamp else 0, _stream())
    _lib.check(rc, "dnmf_background_subtract")
    return out


BACKGROUND_RANKS = (2, 8)    # the R of K23's entries; one component is K19


def _rank_rows(fn, name, t, n, n_name):
    """(R, ...) fp32 CUDA values as R rows of ``n`` floats with unit inner stride -> (rows (R, n), R)."""
    if not isinstance(t, torch.Tensor) or t.dim() < 2:
        raise ValueError(f"{fn}: {name} holds R rows of {n} {n_name}")
    t = t.reshape(t.shape[0], -1)
    _rows(t, fn, name)
    if t.shape[1] != n:
        raise ValueError(f"{fn}: {name} holds R rows of {n} {n_name}, got {tuple(t.shape)}")
    return t, t.shape[0]


def _check_rank(fn, R, inner=1):
    if not BACKGROUND_RANKS[0] <= R <= BACKGROUND_RANKS[1]:
        raise ValueError(f"{fn}: {R} components ({BACKGROUND_RANKS[0]} .. {BACKGROUND_RANKS[1]}; one component is K19)")
    if int(inner) < 1:
        raise ValueError(f"{fn}: inner={inner} sweeps")


def background_state_rank(sz, B, rank, segment=0, device="cuda"):
    """An empty state for ``background_accum_rank`` calls of up to ``B`` frames each; pass it with ``first=True``."""
    X, Y, Z = (int(s) for s in sz)
    need = _need(_lib.load(), "dnmf_background_accum_rank_workspace", X * Y * Z, int(B), int(rank), int(segment))
    return _workspace(None, need, device)


def _dots_rank(frames, b, f, sub, fid, B, P, R, inner):
    """The launch of ``background_dots_rank`` on checked arguments; ``f`` (R, B) rows are the start and receive the result."""
    dev = frames.device
    lib = _lib.load()
    ws = _scratch(_need(lib, "dnmf_background_dots_rank_workspace", P, B, R), dev)
    num = torch.empty((R, B), dtype=torch.float64, device=dev)
    q = torch.empty((R, R), dtype=torch.float64, device=dev)
    with _timed("background_dots_rank"):
        rc = lib.dnmf_background_dots_rank(*_pass_rows(frames, sub, fid, P), b.data_ptr(), _ld(b, P), R, P, B, int(inner), f.data_ptr(),
                                           _ld(f, B), num.data_ptr(), q.data_ptr(), ws.data_ptr(), _nbytes(ws), _stream())
    _lib.check(rc, "dnmf_background_dots_rank")
    return f, num, q


def background_dots_rank(frames, b, f, sub=None, frame_ids=None, inner=3):
    """K23, the f half-step of a rank-R background (2 <= R <= 8).  frames, ``sub``, ``frame_ids`` as ``background_dots`` takes
    them; ``b`` R images (R, ...) of P voxels each, ``f`` (R, B) the current time courses of the frames of the call, both fp32 CUDA
    -> ``(f_new (R, B), num (R, B), q (R, R))``: ``num[j, t] = sum_p b_j[p] (frames - sub)[t, p]`` and ``q = B B^T`` in float64, and
    per frame ``inner`` cyclic sweeps ``f_j <- max(0, (num_j - sum_{i != j} q_ji f_i) / q_jj)`` (0 where q_jj == 0) in float64 from
    ``f``, rounded once to fp32 (tests/background_rank_restatement.py).  One pass over the movie whatever R is.  ``f`` is not
    changed.  Float64 sums in a fixed order: the same input gives the same bits."""
    fn = "background_dots_rank"
    if not isinstance(b, torch.Tensor) or b.dim() < 2:
        raise ValueError(f"{fn}: b holds R images")
    P = b[0].numel()
    b, R = _rank_rows(fn, "b", b, P, "voxels")
    _check_rank(fn, R, inner)
    fid, B = _frame_rows(fn, frames, sub, frame_ids, P)
    f, Rf = _rank_rows(fn, "f", f, B, "frames (one value for each frame of the call)")
    if Rf != R:
        raise ValueError(f"{fn}: {R} images but {Rf} time courses")
    return _dots_rank(frames, b, f.clone(), sub, fid, B, P, R, inner)


def background_accum_rank(frames, f, sz, b=None, sub=None, frame_ids=None, state=None, first=True, finish=True, segment=0, inner=3):
    """K23, the b half-step of a rank-R background.  frames, ``sub``, ``frame_ids``, ``state`` / ``first`` / ``finish`` /
    ``segment`` as ``background_accum`` takes them; ``f`` (R, B) fp32 CUDA, the time courses of the frames of the call; ``b``
    (R, X, Y, Z) the current images (None: zeros), read by the finishing call only -> ``((b_new, num, w) or None, state)``:
    over the frames seen since the state was reset ``num[j, p] = sum_t f_j[t] (frames - sub)[t, p]`` ((R, X, Y, Z) float64) and
    ``w = F F^T`` ((R, R) float64), and per voxel ``inner`` cyclic sweeps from ``b`` as in ``background_dots_rank``, rounded once to
    fp32 ((R, X, Y, Z)).  ``b`` is not changed.  Every call on one state has the same volume and R."""
    fn = "background_accum_rank"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows(fn, frames, sub, frame_ids, P)
    f, R = _rank_rows(fn, "f", f, B, "frames (one value for each frame of the call)")
    _check_rank(fn, R, inner)
    dev = frames.device
    lib = _lib.load()
    need = _need(lib, "dnmf_background_accum_rank_workspace", P, B, R, int(segment))
    state = _stream_state(fn, state, need, first, dev)
    out = num = w = None
    if finish:
        if b is None:
            out = torch.zeros((R, X, Y, Z), dtype=torch.float32, device=dev)
        else:
            rows, Rb = _rank_rows(fn, "b", b, P, "voxels")
            if Rb != R:
                raise ValueError(f"{fn}: {R} time courses but {Rb} images")
            out = rows.clone().reshape(R, X, Y, Z)
        num = torch.empty((R, X, Y, Z), dtype=torch.float64, device=dev)
        w = torch.empty((R, R), dtype=torch.float64, device=dev)
    with _timed("background_accum_rank"):
        rc = lib.dnmf_background_accum_rank(*_pass_rows(frames, sub, fid, P), f.data_ptr(), _ld(f, B), R, P, B, 1 if first else 0,
                                            1 if finish else 0, int(segment), int(inner), state.data_ptr(), _nbytes(state), _ptr(out), P,
                                            _ptr(num), _ptr(w), _stream())
    _lib.check(rc, "dnmf_background_accum_rank")
    return ((out, num, w) if finish else None), state


def background_subtract_rank(frames, b, f, frame_ids=None, times=None, out=None, clamp=True):
    """K23.  ``out[j] = fp32(float64(frames[row j]) - sum_c float64(b_c) float64(f_c[t_j]))``, the products added with c ascending,
    ``max(., 0)`` with ``clamp``: ``b`` R images (R, ...), ``f`` (R, T); everything else as ``background_subtract``."""
    fn = "background_subtract_rank"
    if not isinstance(b, torch.Tensor) or b.dim() < 2:
        raise ValueError(f"{fn}: b holds R images")
    P = b[0].numel()
    b, R = _rank_rows(fn, "b", b, P, "voxels")
    if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] != R:
        raise ValueError(f"{fn}: f is (R={R}, T)")
    _rows(f, fn, "f")
    _check_rank(fn, R)
    nf = f.shape[1]
    fid, tt, B = _subtract_rows(fn, frames, frame_ids, times, P)
    out = _out_rows(fn, out, B, P, frames.device)
    lib = _lib.load()
    with _timed("background_subtract_rank"):
        rc = lib.dnmf_background_subtract_rank(frames.data_ptr(), _ld(frames, P), _ptr(fid), b.data_ptr(), _ld(b, P), f.data_ptr(),
                                               _ld(f, nf), R, nf, _ptr(tt), P, B, out.data_ptr(), _ld(out, P), 1 if clamp else 0,
                                               _stream())
    _lib.check(rc, "dnmf_background_subtract_rank")
    return out


def _pieces(P, T, piece):
    """The cuts of T resident rows into pieces of ``piece`` frames (None: at most 1 GiB of frames)."""
    if piece is None:
        piece = max(1, (1 << 30) // (4 * P))
    piece = max(1, min(int(piece), T))
    return [(s, min(T, s + piece)) for s in range(0, T, piece)]


def background_fit_rank(frames, sz, iters, rank, sub_fn=None, piece=None, inner=3):
    """The rank-R background of resident rows (K23), 2 <= R <= 8: R images and R time courses -> ``(b (R, X, Y, Z), f (R, T))`` fp32
    CUDA, all >= 0 (tests/background_rank_restatement.py: ``fit``).  F starts as the indicators of R contiguous blocks of the
    rows, b from one b-step on them (the clipped block means); then ``iters`` times the pair (``background_dots_rank``,
    ``background_accum_rank``) with ``inner`` coordinate sweeps per frame and per voxel, then per component the scale that makes
    mean(f_j) = 1.  ``sub_fn`` and ``piece`` as ``background_fit`` takes them; ``sub_fn`` is called once more per piece, for the
    start.  ``rank=1`` is ``background_fit``, whatever ``inner`` is.  No host synchronisation."""
    if int(rank) != rank or rank < 1:
        raise ValueError(f"background_fit_rank: rank={rank!r}")
    if rank == 1:
        return background_fit(frames, sz, iters, sub_fn=sub_fn, piece=piece)
    if int(iters) < 1:
        raise ValueError(f"background_fit_rank: iters={iters}")
    X, Y, Z = (int(s) for s in sz)
    P, T, R = X * Y * Z, frames.shape[0], int(rank)
    cuts = _pieces(P, T, piece)
    dev = frames.device
    _check_rank("background_fit_rank", R, inner)
    if R > T:
        raise ValueError(f"background_fit_rank: rank={R} for {T} frames")
    _rows(frames, "background_fit_rank", "frames", P, f" and rows of {P} floats")
    # the start: component j owns the contiguous block of frames with (t R) // T == j
    t = torch.arange(T, device=dev)
    f = torch.zeros((R, T), dtype=torch.float32, device=dev)
    f[(t * R) // T, t] = 1.0
    b = torch.zeros((R, X, Y, Z), dtype=torch.float32, device=dev)
    state = None

    def sub(s, e):
        return None if sub_fn is None else sub_fn(s, e)

    def b_step(b):
        nonlocal state
        for n, (s, e) in enumerate(cuts):
            res, state = background_accum_rank(frames[s:e], f[:, s:e], (X, Y, Z), b=b, sub=sub(s, e), state=state, first=n == 0,
                                               finish=e == T, inner=inner)
        return res[0]

    b = b_step(b)
    for _ in range(int(iters)):
        for s, e in cuts:
            m = sub(s, e)
            fid, B = _frame_rows("background_fit_rank", frames[s:e], m, None, P)
            _dots_rank(frames[s:e], b.reshape(R, P), f[:, s:e], m, fid, B, P, R, inner)      # in place, on the rows of f
        b = b_step(b)
    scale = f.mean(dim=1)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return b.mul_(scale[:, None, None, None]), f.div_(scale[:, None])


def background_fit(frames, sz, iters, sub_fn=None, piece=None):
    """The rank-1 background of resident rows: ``iters`` times the pair (``background_dots``, ``background_accum``) from b = 1,
    then the scale that makes mean(f) = 1 -> ``(b (X, Y, Z), f (T,))`` fp32 CUDA, both >= 0 (tests/background_restatement.py:
    ``fit``).  The rows go through in pieces of ``piece`` frames (None: at most 1 GiB of frames); ``sub_fn(s, e)`` returns the
    rows to subtract from frames ``s:e`` ((e - s, ld >= P) fp32 CUDA, e.g. the model's prediction), so that they are never
    held for the whole movie -- it is called twice per iteration and piece.  No host synchronisation."""
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    T = frames.shape[0]
    if int(iters) < 1:
        raise ValueError(f"background_fit: iters={iters}")
    cuts = _pieces(P, T, piece)
    dev = frames.device
    b = torch.ones((X, Y, Z), dtype=torch.float32, device=dev)
    f = torch.empty((T,), dtype=torch.float32, device=dev)
    state = None
    for _ in range(int(iters)):
        for s, e in cuts:
            f[s:e] = background_dots(frames[s:e], b, sub=None if sub_fn is None else sub_fn(s, e))[0]
        for n, (s, e) in enumerate(cuts):
            res, state = background_accum(frames[s:e], f[s:e], (X, Y, Z), sub=None if sub_fn is None else sub_fn(s, e), state=state,
                                          first=n == 0, finish=e == T)
        b = res[0]
    scale = f.mean()
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return b.mul_(scale), f.div_(scale)


def clean_traces(traces, fps, sigma_threshold=10, detrend_mode=2, interp_method=None, smooth_method=None, smooth_window=None,
                 trim=True, floor=0.01, workspace=None):
    """K20, the trace clean-up of tests/traces_restatement.py (``clean_traces``: mask, single-frame outliers, bleach detrend, dF/F0,
    gap filling, smoothing, rescale) on the GPU.  traces (K, T) fp32 CUDA rows with unit inner stride -- any row stride, no copy
    is made and the input is only read -> ``(traces (K, T) fp32, scales (K,), offsets (K,), info)`` on the GPU; ``info``: ``a``,
    ``b``, ``F0`` (float64), ``fitted`` (bool), ``n_outliers`` (int32) per neuron and ``workspace``.  ``sigma_threshold`` None or
    0: no outlier step; ``interp_method`` None or 'linear'; ``smooth_method`` None, 'movmean' or 'movmedian' over ``smooth_window``
    frames ('causal', 'high' and 'low' name filters the reference does not contain: NotImplementedError).  Float64 inside, one
    rounding to fp32, sums in a fixed order: the same input gives the same bits.  No host synchronisation."""
    if traces.dim() != 2:
        raise ValueError(f"clean_traces: traces are (K, T), got {tuple(traces.shape)}")
    _rows(traces, "clean_traces", "traces")
    if interp_method is not None and interp_method != "linear":
        raise ValueError(f"clean_traces: interp_method={interp_method!r}: 'linear' or None")
    if smooth_method in ("causal", "high", "low"):
        raise NotImplementedError(f"clean_traces: smooth_method={smooth_method!r} names a filter (causalBandpassFilter / "
                                  "highpassFilter / lowpassFilter) that the reference does not contain")
    if smooth_method is not None and smooth_method not in ("movmean", "movmedian"):
        raise ValueError(f"clean_traces: smooth_method={smooth_method!r}: 'movmean', 'movmedian' or None")
    smooth = 0 if smooth_method is None or smooth_window is None else (1 if smooth_method == "movmean" else 2)
    K, T = traces.shape
    dev = traces.device
    lib = _lib.load()
    need = _need(lib, "dnmf_clean_traces_workspace", K, T)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(((need + 7) // 8,), dtype=torch.float64, device=dev)
    out = torch.empty((K, T), dtype=torch.float32, device=dev)
    f64 = torch.empty((5, K), dtype=torch.float64, device=dev)      # scales, offsets, a, b, F0
    i32 = torch.empty((2, K), dtype=torch.int32, device=dev)        # fitted, n_outliers
    with _timed("clean_traces"):
        rc = lib.dnmf_clean_traces(traces.data_ptr(), _ld(traces, T), K, T, float(fps),
                                   0.0 if sigma_threshold is None else float(sigma_threshold), int(detrend_mode),
                                   0 if interp_method is None else 1, smooth, int(smooth_window) if smooth else 0, 1 if trim else 0,
                                   float(floor), out.data_ptr(), T, f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(),
                                   f64[3].data_ptr(), f64[4].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), workspace.data_ptr(),
                                   _nbytes(workspace), _stream())
    _lib.check(rc, "dnmf_clean_traces")
    info = dict(a=f64[2], b=f64[3], F0=f64[4], fitted=i32[0] != 0, n_outliers=i32[1], workspace=workspace)
    return out, f64[0], f64[1], info


def _per_trace(v, K, dev, fn, name, lo=None, hi=None, closed_lo=False):
    """An option of ``deconvolve_traces`` -> a (K,) float64 tensor on ``dev`` (NaN: estimate) or None.  A number is checked
    against its range here; the entries of an array are judged per trace by the kernel."""
    if v is None:
        return None
    if not isinstance(v, torch.Tensor) and not hasattr(v, "__len__"):
        x = float(v)
        if x == x and ((lo is not None and (x < lo if closed_lo else x <= lo)) or (hi is not None and x >= hi)):
            raise ValueError(f"{fn}: {name}={x}")
        return torch.full((K,), x, dtype=torch.float64, device=dev)
    t = torch.as_tensor(v).to(device=dev, dtype=torch.float64).contiguous()
    if t.shape != (K,):
        raise ValueError(f"{fn}: {name} is a number or one value per trace ({K}), got {tuple(t.shape)}")
    return t


def deconvolve_traces(traces, g=None, penalty=None, baseline=None, noise=None, baseline_percentile=10.0, workspace=None):
    """K21, the spike deconvolution of tests/deconv_restatement.py (``deconvolve_traces``) on the GPU: per trace y the c >= 0 that
    minimises 1/2 sum w (y - b - c)^2 + penalty sum s with s_t = c_t - g c_{t-1} >= 0, w = 0 on the frames that are not finite
    (what ``clean_traces`` masks).  traces (K, T) fp32 CUDA rows with unit inner stride -- any row stride, no copy is made and the
    input is only read -> ``(c (K, T) fp32, s (K, T) fp32, info)`` on the GPU; ``info``: ``g``, ``penalty``, ``baseline``,
    ``noise``, ``rss`` (float64), ``n_valid``, ``n_pools`` (int32), ``ok`` (bool) per trace and ``workspace``.  Each of ``g``,
    ``penalty``, ``baseline``, ``noise``: None (estimate it), a number, or a ``(K,)`` array or tensor whose NaN entries are
    estimated.  The estimated baseline is the ``baseline_percentile``-th percentile of the valid frames: it sits below the true
    baseline by a fraction of the noise.  A trace that cannot be treated (too few valid frames, no decay in (0, 1), ...) has
    ``ok`` False and NaN rows.  Float64 inside, one rounding to fp32, sums in a fixed order: the same input gives the same bits.
    One launch, no host synchronisation."""
    fn = "deconvolve_traces"
    if traces.dim() != 2:
        raise ValueError(f"{fn}: traces are (K, T), got {tuple(traces.shape)}")
    _rows(traces, fn, "traces")
    K, T = traces.shape
    dev = traces.device
    if not 0.0 <= float(baseline_percentile) <= 100.0:
        raise ValueError(f"{fn}: baseline_percentile={baseline_percentile}")
    opts = [_per_trace(g, K, dev, fn, "g", lo=0.0, hi=1.0), _per_trace(penalty, K, dev, fn, "penalty", lo=0.0, closed_lo=True),
            _per_trace(baseline, K, dev, fn, "baseline"), _per_trace(noise, K, dev, fn, "noise", lo=0.0, closed_lo=True)]
    lib = _lib.load()
    need = _need(lib, "dnmf_deconvolve_traces_workspace", K, T)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(((need + 7) // 8,), dtype=torch.float64, device=dev)
    c = torch.empty((K, T), dtype=torch.float32, device=dev)
    s = torch.empty((K, T), dtype=torch.float32, device=dev)
    out = torch.empty((K, 8), dtype=torch.float64, device=dev)
    with _timed("deconvolve_traces"):
        rc = lib.dnmf_deconvolve_traces(traces.data_ptr(), _ld(traces, T), K, T, *[_ptr(o) for o in opts], float(baseline_percentile),
                                        c.data_ptr(), s.data_ptr(), T, out.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                        _stream())
    _lib.check(rc, "dnmf_deconvolve_traces")
    info = dict(g=out[:, 0], penalty=out[:, 1], baseline=out[:, 2], noise=out[:, 3], rss=out[:, 4], n_valid=out[:, 5].to(torch.int32),
                n_pools=out[:, 6].to(torch.int32), ok=out[:, 7] != 0, workspace=workspace)
    return c, s, info


AR1_MAX_FRAMES = 6144   # K32: POOL_LDS_FRAMES of csrc/ar1_pools.hpp, where the number and its reason live
AR1_MAX_K = 4096


def trace_colours(nbr_or_pattern):
    """K32's colours of the overlap graph, on the host (numpy) -> ``(colour (K,) int32, n_colours)``: a greedy colouring, k
    ascending, the smallest colour no neighbour holds.  ``nbr_or_pattern``: a neighbour table (K, NN) of integers (row k names the
    columns of G that can be non-zero in row k; entries outside [0, K) are padding), or a (K, K) bool pattern; array or tensor.  k
    and l are neighbours when either names the other.  Neurons of one colour share no Gram entry."""
    a = nbr_or_pattern.detach().cpu().numpy() if isinstance(nbr_or_pattern, torch.Tensor) else np.asarray(nbr_or_pattern)
    if a.ndim != 2:
        raise ValueError(f"trace_colours: a neighbour table (K, NN) or a pattern (K, K), got {a.shape}")
    K = a.shape[0]
    if a.dtype == np.bool_:
        if a.shape[1] != K:
            raise ValueError(f"trace_colours: a pattern is (K, K), got {a.shape}")
        adj = a.copy()
    else:
        adj = np.zeros((K, K), dtype=bool)
        rows = np.repeat(np.arange(K), a.shape[1])
        cols = a.reshape(-1).astype(np.int64)
        ok = (cols >= 0) & (cols < K)
        adj[rows[ok], cols[ok]] = True
    adj |= adj.T
    adj[np.arange(K), np.arange(K)] = False
    colour = np.full(K, -1, dtype=np.int32)
    for k in range(K):
        taken = np.zeros(K + 1, dtype=bool)
        held = colour[adj[k]]
        taken[held[held >= 0]] = True
        colour[k] = int(np.flatnonzero(~taken)[0])
    return colour, (int(colour.max()) + 1 if K else 0)


def _ar1_lists(nbr, K):
    """A neighbour table as K32 walks it: row k's valid columns and k itself, ascending, each once, padded with -1 (A1 of
    tests/ar1_restatement.py).  Device work only."""
    n = nbr.to(torch.int64)
    me = torch.arange(K, device=n.device, dtype=torch.int64)[:, None]
    n = torch.cat([torch.where((n >= 0) & (n < K), n, torch.full_like(n, K)), me], 1).sort(1).values
    dup = torch.zeros_like(n, dtype=torch.bool)
    dup[:, 1:] = n[:, 1:] == n[:, :-1]
    n = torch.where(dup, torch.full_like(n, K), n).sort(1).values
    return torch.where(n < K, n, torch.full_like(n, -1)).to(torch.int32).contiguous()


def _ar1_check(fn, G, r, C64, nbr):
    _state(fn, C64, torch.float64, "the state", " (K, T)")
    K, T = _gram_against_state(fn, G, r, C64)
    if T > AR1_MAX_FRAMES or K > AR1_MAX_K:
        raise ValueError(f"{fn}: K={K}, T={T}: at most {AR1_MAX_K} neurons and {AR1_MAX_FRAMES} consecutive frames a call (a row's "
                         "pool records live in LDS); a longer run is refused, not cut")
    if nbr is not None and not (isinstance(nbr, torch.Tensor) and nbr.is_cuda and nbr.dim() == 2 and nbr.shape[0] == K
                                and nbr.shape[1] >= 1 and not nbr.dtype.is_floating_point):
        raise ValueError(f"{fn}: nbr must be an integer CUDA tensor of shape (K={K}, NN)")
    return K, T


def _ar1_params(fn, K, dev, g, penalty, baseline):
    """``g``, ``penalty``, ``baseline`` (a number or K of them) as (K,) float64 tensors on ``dev``, checked on the host."""
    out = []
    for name, v in (("g", g), ("penalty", penalty), ("baseline", baseline)):
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if a.shape not in ((), (K,)):
            raise ValueError(f"{fn}: {name} is a number or one value per neuron ({K}), got {a.shape}")
        a = np.broadcast_to(a.astype(np.float64), (K,)).copy()
        if name == "g" and not bool(((a >= 0.0) & (a < 1.0)).all()):
            raise ValueError(f"{fn}: g must lie in [0, 1), got {a[~((a >= 0.0) & (a < 1.0))][:4]}")
        if name == "penalty" and not bool((a >= 0.0).all() and np.isfinite(a).all()):
            raise ValueError(f"{fn}: penalty must be finite and >= 0")
        if name == "baseline" and not bool(np.isfinite(a).all()):
            raise ValueError(f"{fn}: baseline must be finite")
        out.append(torch.from_numpy(a).to(dev))
    return out


def _ar1_step(G, r, C64, ids, g, penalty, baseline, lists, s, counts):
    K, T = C64.shape
    with _timed("ar1_temporal_step"):
        rc = _lib.load().dnmf_ar1_temporal_step(G.data_ptr(), r.data_ptr(), C64.data_ptr(), C64.stride(0), K, T, ids.data_ptr(),
                                                ids.numel(), g.data_ptr(), penalty.data_ptr(), baseline.data_ptr(), _ptr(lists),
                                                0 if lists is None else lists.shape[1], s.data_ptr(), s.stride(0), counts.data_ptr(),
                                                _stream())
    _lib.check(rc, "dnmf_ar1_temporal_step")


def ar1_temporal_step(G, r, C64, ids, g, penalty, baseline, nbr=None, s=None):
    """K32, one launch: the row step A3 of tests/ar1_restatement.py for the neurons ``ids`` (a list, array or tensor of distinct
    indices) on the float64 state ``C64`` (K, T), in place.  G (T, K, K), r (T, K) fp32 Gram data of T consecutive frames in time
    order.  The listed neurons must share no Gram entry (one colour of ``trace_colours``): their steps then do not see each other.
    ``g`` in [0, 1), ``penalty`` >= 0, ``baseline``: a number or (K,) each.  ``nbr`` (K, NN) integers: the columns of G that can be
    non-zero per row (``pack_footprints_lists``); None: all K.  ``s`` (K, T) float64 receives the spikes of the listed rows (a new
    tensor of zeros without it) -> ``(C64, s, counts)``, counts (K, 2) int32: the pools and the frames without weight of the listed
    rows (zero elsewhere)."""
    fn = "ar1_temporal_step"
    K, T = _ar1_check(fn, G, r, C64, nbr)
    dev = C64.device
    idh = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    idh = idh.astype(np.int64).reshape(-1)
    if idh.size < 1 or idh.min() < 0 or idh.max() >= K or np.unique(idh).size != idh.size:
        raise ValueError(f"{fn}: ids are distinct neurons in [0, {K}), at least one")
    g, penalty, baseline = _ar1_params(fn, K, dev, g, penalty, baseline)
    if s is None:
        s = torch.zeros((K, T), dtype=torch.float64, device=dev)
    elif not (s.is_cuda and s.dtype == torch.float64 and tuple(s.shape) == (K, T) and s.stride(1) == 1):
        raise ValueError(f"{fn}: s must be float64 CUDA ({K}, {T}) with unit inner stride")
    counts = torch.zeros((K, 2), dtype=torch.int32, device=dev)
    _ar1_step(G, r, C64, torch.from_numpy(idh.astype(np.int32)).to(dev), g, penalty, baseline,
              None if nbr is None else _ar1_lists(nbr, K), s, counts)
    return C64, s, counts


def ar1_temporal(G, r, C, g, penalty=0.0, baseline=0.0, sweeps=1, nbr=None):
    """K32, the AR(1)-constrained trace update of tests/ar1_restatement.py (``ar1_temporal``) on the GPU: ``sweeps`` sweeps of block
    coordinate descent over the neurons on

        F(C) = sum_t (1/2 c_t^T G_t c_t - r_t^T c_t) + sum_k penalty_k sum_t s_kt,   x = C[k] - baseline_k,  s_kt = x_t - g_k x_{t-1} >= 0

    (s_k0 = x_0 >= 0).  A row step replaces neuron k's row by the deconvolution of its own residual trace, every frame weighted by
    G_t[k,k]: the exact minimiser of F over that row (K21's pool-adjacent-violators with weights).  A sweep goes colour by colour of
    ``trace_colours`` (of ``nbr``, else of the pattern of G, which costs one pass over G), one launch a colour.  G (T, K, K),
    r (T, K) fp32: the Gram data of T consecutive frames in time order; C (K, T) fp32 CUDA with unit inner stride, any row stride,
    updated in place: the float64 state is kept across the sweeps and rounded to fp32 once at the end.  ``g`` in [0, 1) (0: the
    plain non-negative step for that neuron), ``penalty`` >= 0, ``baseline``: a number or (K,) each.  -> ``(C, s, info)``: s (K, T)
    float64, the spikes; ``info``: ``colour`` (K,) int32 numpy and ``n_colours``, ``n_pools`` and ``n_weightless`` (K,) int32 of
    every row's last step, and ``state``, the float64 (K, T) state before the rounding.  T <= ``AR1_MAX_FRAMES`` and
    K <= ``AR1_MAX_K``: anything larger is refused.  Sums in a fixed order without floating-point atomics: the same input gives the same bits."""
    fn = "ar1_temporal"
    if not (isinstance(C, torch.Tensor) and C.dim() == 2):
        raise ValueError(f"{fn}: C is a (K, T) tensor")
    _rows(C, fn, "C")
    if int(sweeps) != sweeps or sweeps < 0:
        raise ValueError(f"{fn}: sweeps={sweeps!r}, a whole number >= 0")
    state = C.double().contiguous()
    K, T = _ar1_check(fn, G, r, state, nbr)
    dev = C.device
    g, penalty, baseline = _ar1_params(fn, K, dev, g, penalty, baseline)
    colour, n_colours = trace_colours(nbr if nbr is not None else ((G != 0).any(0)).cpu().numpy())
    groups = [torch.from_numpy(np.flatnonzero(colour == c).astype(np.int32)).to(dev) for c in range(n_colours)]
    lists = None if nbr is None else _ar1_lists(nbr, K)
    s = torch.zeros((K, T), dtype=torch.float64, device=dev)
    counts = torch.zeros((K, 2), dtype=torch.int32, device=dev)
    for _ in range(int(sweeps)):
        for ids in groups:
            _ar1_step(G, r, state, ids, g, penalty, baseline, lists, s, counts)
    C.copy_(state)
    return C, s, dict(colour=colour, n_colours=n_colours, n_pools=counts[:, 0], n_weightless=counts[:, 1], state=state)


def histogram_match(a, b, nbins, nonneg=False, out=None, quantiles=False):
    """K25, the quantile-matched rescaling of tests/histmatch_restatement.py (``histogram_match``) on the GPU: per row the affine
    map ``a beta0 + beta1`` that carries the ``nbins`` quantiles of the moving trace ``a`` onto those of the reference trace ``b``
    (least squares on the matched quantiles; ``nonneg``: under beta0 >= 0 and beta1 >= 0).  a (K, Ta) and b (K, Tb) -- or
    (Tb,), one row shared by all -- fp32 CUDA rows with unit inner stride: any row stride, no copy is made and the inputs are only
    read; samples that are not finite count for nothing and the two sides need neither the same length nor the same mask ->
    ``(out (K, Ta) fp32, beta (K, 2) float64, distance (K,) float64, info (K, 3) int32: na, nb, ok)`` on the GPU, and with
    ``quantiles`` also ``qa`` and ``qb`` (K, nbins) float64.  ``out``: rows to write into (K, Ta), else new ones.  A row without
    a valid sample on either side has ok = 0 and NaN results.  Ta, Tb <= 16 384, 2 <= nbins <= 1024, K <= 18 432: anything else
    is refused.  Float64 inside, one rounding to fp32, sums in a fixed order: the same input gives the same bits.  One launch,
    no host synchronisation."""
    fn = "histogram_match"
    if a.dim() != 2 or b.dim() not in (1, 2):
        raise ValueError(f"{fn}: a is (K, Ta) and b (K, Tb) or (Tb,), got {tuple(a.shape)} and {tuple(b.shape)}")
    _rows(a, fn, "a")
    _rows(b, fn, "b")
    K, Ta = a.shape
    Tb = b.shape[-1]
    dev = a.device
    if b.device != dev:
        raise ValueError(f"{fn}: a is on {dev}, b on {b.device}")
    if b.dim() == 2 and b.shape[0] != K:
        raise ValueError(f"{fn}: b must hold one row for each of the {K} rows of a, or be one row (Tb,); got {tuple(b.shape)}")
    if out is None:
        out = torch.empty((K, Ta), dtype=torch.float32, device=dev)
    else:
        _rows(out, fn, "out")
        if out.shape != (K, Ta) or out.device != dev:
            raise ValueError(f"{fn}: out must be {(K, Ta)} on {dev}, got {tuple(out.shape)} on {out.device}")
    nbins = int(nbins)
    lib = _lib.load()
    beta = torch.empty((K, 2), dtype=torch.float64, device=dev)
    distance = torch.empty((K,), dtype=torch.float64, device=dev)
    info = torch.empty((K, 3), dtype=torch.int32, device=dev)
    q = torch.empty((2, K, max(nbins, 0)), dtype=torch.float64, device=dev) if quantiles else None
    with _timed("histogram_match"):
        rc = lib.dnmf_histogram_match(a.data_ptr(), _ld(a, Ta), Ta, b.data_ptr(), 0 if b.dim() == 1 else _ld(b, Tb), Tb, K, nbins,
                                      1 if nonneg else 0, out.data_ptr(), _ld(out, Ta), beta.data_ptr(), distance.data_ptr(),
                                      info.data_ptr(), _ptr(q[0] if quantiles else None), _ptr(q[1] if quantiles else None), _stream())
    _lib.check(rc, "dnmf_histogram_match")
    return (out, beta, distance, info, q[0], q[1]) if quantiles else (out, beta, distance, info)


def high_pass_taps(gSig):
    """The (n, n) float64 numpy kernel of the reference's ``high_pass_filter_space`` (MotionCorrect.py:1263-1269):
    ``n = (3 gSig[0]) // 2 * 2 + 1`` (entry 0 decides, the kernel is square), ``cv2.getGaussianKernel(n, gSig[0])`` written out
    (``exp(-x^2 / (2 sigma^2))`` at ``x = i - (n - 1) / 2`` over its sum), its outer product with itself, the mean of the entries
    ``>= ker2D[:, 0].max()`` (a disc) subtracted from those entries and every other entry set to 0: the kernel sums to zero.
    The Gaussian is evaluated in OpenCV's order of operations -- ``exp((-0.5 / sigma^2) x x)``, times the reciprocal of the sum --
    because the disc's rim has exact ties (6^2 + 8^2 = 10^2 at gSig 7) that the last bit decides: 309 taps this way, 317 with
    ``-x x / (2 sigma^2)``."""
    import numpy as np
    try:
        g = [float(v) for v in gSig]
    except TypeError:
        g = [float(gSig)]
    if not g or any(not np.isfinite(v) or v <= 0 for v in g):
        raise ValueError(f"high_pass_taps: gSig must be positive and finite, got {gSig!r}")
    n = int((3 * g[0]) // 2 * 2 + 1)
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    ker = np.exp((-0.5 / (g[0] * g[0])) * x * x)
    ker = ker * (1.0 / ker.sum())
    ker2D = ker[:, None] * ker[None, :]
    nz = np.nonzero(ker2D >= ker2D[:, 0].max())
    zz = np.nonzero(ker2D < ker2D[:, 0].max())
    ker2D[nz] -= ker2D[nz].mean()
    ker2D[zz] = 0
    return ker2D


_HIGH_PASS_TAPS = {}


def _span(t, B, P):
    """[first, last) byte addresses of rows ``t`` (the first B rows, or all of them for B = None)."""
    rows = t.shape[0] if B is None else B
    return t.data_ptr(), t.data_ptr() + 4 * ((rows - 1) * _ld(t, P) + P)


def high_pass_frames(frames, sz, gSig, frame_ids=None, out=None, taps=None):
    """K22.  frames (rows, ld >= X Y Z) fp32 CUDA rows -> ``out`` (B, P) fp32 CUDA rows (or (>= B, ldo >= P) given; it may not
    overlap ``frames``): every frame correlated slice by slice with ``high_pass_taps(gSig)`` rounded to fp32, reflected at the
    borders with period 2 N (cv2's BORDER_REFLECT), taps that are zero not applied -- ``high_pass_filter_space`` of the
    reference.  ``frame_ids``: the rows of ``frames`` to take (None: all, in order).  ``taps``: an (n, n) array to use in place of
    the kernel of ``gSig`` (n odd, at most 31).  fp32 FMAs in a fixed order: the same input gives the same bits."""
    import numpy as np
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows("high_pass_frames", frames, None, frame_ids, P)
    dev = frames.device
    if taps is None:
        k = high_pass_taps(gSig)
        key = (k.tobytes(), str(dev))
        if key not in _HIGH_PASS_TAPS:
            _HIGH_PASS_TAPS[key] = torch.from_numpy(k.astype(np.float32)).to(dev)
        tp = _HIGH_PASS_TAPS[key]
    else:
        tp = torch.as_tensor(np.asarray(taps.cpu() if torch.is_tensor(taps) else taps, dtype=np.float32)).to(dev).contiguous()
        if tp.dim() != 2 or tp.shape[0] != tp.shape[1]:
            raise ValueError(f"high_pass_frames: taps are (n, n), got {tuple(tp.shape)}")
    out = _out_rows("high_pass_frames", out, B, P, dev)
    if B >= 1 and P >= 1:
        (f0, f1), (o0, o1) = _span(frames, None, P), _span(out, B, P)
        if o0 < f1 and f0 < o1:
            raise ValueError("high_pass_frames: out overlaps frames (a voxel's neighbours are read after it is written)")
    lib = _lib.load()
    with _timed("high_pass_frames"):
        rc = lib.dnmf_high_pass_frames(frames.data_ptr(), _ld(frames, P), _ptr(fid), _int3((X, Y, Z)), B, tp.data_ptr(), tp.shape[0],
                                       out.data_ptr(), _ld(out, P), _stream())
    _lib.check(rc, "dnmf_high_pass_frames")
    return out


COMPONENT_MAX_VOXELS = 4096   # the largest box of K24, K26, K27 and K28 (csrc/boxes.hpp: BOX_MAX_VOXELS)


def _boxes(fn, boxes, sz, n=None, limit=COMPONENT_MAX_VOXELS, noun="box", dev=None, check=True):
    """``boxes`` (``n``, 6) -- None: (M, 6), M >= 1 -- as the box kernels take them -> (the host int32 copy, its copy on ``dev``,
    the voxels of each box, int64).  With ``check`` every box lies inside the volume ``sz``, is not empty and holds at most
    ``limit`` voxels, ``noun`` naming it in that message; without, the library's own check of the host copy speaks."""
    X, Y, Z = (int(s) for s in sz)
    bh = torch.as_tensor(boxes).detach().to("cpu", torch.int32).contiguous()
    if (bh.dim() != 2 or bh.shape[1] != 6 or bh.shape[0] < 1) if n is None else tuple(bh.shape) != (n, 6):
        raise ValueError(f"{fn}: boxes must be ({'M' if n is None else n}, 6), got {tuple(bh.shape)}")
    lo, hi = bh[:, 0::2].long(), bh[:, 1::2].long()
    nvox = (hi - lo + 1).prod(1)
    if check:
        wrong = ((lo < 0) | (hi >= torch.tensor([X, Y, Z])) | (lo > hi)).any(1)
        if bool(wrong.any()):
            k = int(torch.nonzero(wrong)[0])
            raise ValueError(f"{fn}: box {k} = {bh[k].tolist()} is empty or outside the volume {X}x{Y}x{Z}")
        if int(nvox.max()) > limit:
            raise ValueError(f"{fn}: {noun} {int(nvox.argmax())} holds {int(nvox.max())} voxels, at most {limit}")
    return bh, (bh if dev is None else bh.to(dev)), nvox


def _a_rows(fn, A_rows, P):
    """The footprints as fp32 CUDA rows (K, >= ``P``) -> K."""
    if A_rows.dim() != 2:
        raise ValueError(f"{fn}: A_rows are rows (K, ld), got {tuple(A_rows.shape)}")
    _rows(A_rows, fn, "A_rows", P, f" and rows of {P} floats")
    return A_rows.shape[0]


def component_boxes(A, sz, floor=1e-3, margin=2):
    """(K, 6) int32 ``(x0, x1, y0, y1, z0, z1)``, inclusive: per neuron the bounding box of ``A[:, k] > floor max A[:, k]``,
    grown by ``margin`` voxels and cut to the volume -- the boxes ``component_stats`` takes.  ``A`` (..., K), on its device.  A
    footprint that is zero everywhere gets the whole volume."""
    X, Y, Z = (int(s) for s in sz)
    K = A.shape[-1]
    A4 = A.reshape(X, Y, Z, K)
    on = A4 > float(floor) * A4.amax(dim=(0, 1, 2))
    boxes = torch.empty((K, 6), dtype=torch.int32, device=A.device)
    for d, S in enumerate((X, Y, Z)):
        hit = on.any(dim=tuple(i for i in range(3) if i != d))                         # (S, K)
        idx = torch.arange(S, device=A.device)[:, None]
        lo = torch.where(hit, idx, S - 1).amin(0)
        hi = torch.where(hit, idx, 0).amax(0)
        none = ~hit.any(0)
        boxes[:, 2 * d] = torch.where(none, 0, (lo - int(margin)).clamp_min(0))
        boxes[:, 2 * d + 1] = torch.where(none, S - 1, (hi + int(margin)).clamp_max(S - 1))
    return boxes


def component_snr(raw, w):
    """(K,) float64: (mean of raw[k] over the valid frames with w[k] > 0 - median of raw[k] over the valid frames) / noise_k,
    noise_k = MAD(diff(raw[k, valid])) / (0.6745 sqrt 2), the estimator K21 documents; a frame is valid where ``raw`` is
    finite.  NaN with fewer than 4 valid frames, without a valid active frame or with a zero noise.  ``raw`` (K, T) from
    ``component_stats``, ``w`` (K, T) its weights.  Float64 torch on the (K, T) arrays: O(K T), not a hot path."""
    raw = raw.double()
    K = raw.shape[0]
    out = torch.full((K,), float("nan"), dtype=torch.float64, device=raw.device)
    ok = torch.isfinite(raw)
    act = ok & (w > 0)
    scale = 0.6745 * 2.0 ** 0.5
    for k in torch.nonzero((ok.sum(1) >= 4) & act.any(1)).reshape(-1).tolist():
        x = raw[k, ok[k]]
        d = x[1:] - x[:-1]
        noise = torch.quantile((d - torch.quantile(d, 0.5)).abs(), 0.5) / scale
        out[k] = torch.where(noise > 0, (raw[k, act[k]].mean() - torch.quantile(x, 0.5)) / noise, out[k])
    return out


def component_stats(frames, sz, A_rows, boxes, C, w, sub=None, frame_ids=None, state=None, first=True, finish=True, segment=0):
    """K24.  Per-component statistics on registered frames -> ``(dict, state)``.  ``frames`` (rows, ld >= P) fp32 CUDA rows in
    footprint coordinates, ``A_rows`` (K, >= P) fp32 the footprints as rows, ``boxes`` (K, 6) int32 inclusive boxes of at most
    4096 voxels (``component_boxes``), ``C`` and ``w`` (K, B) fp32 the traces and the weights >= 0 of the call's frames, in
    their order; ``sub`` (B, ld >= P) fp32 rows: what the model predicts (row j for the j-th frame), None: nothing;
    ``frame_ids``: the rows of ``frames`` to take.  With e_t = frames_t - sub_t + a C[k, t] on the box of neuron k, the
    float64 CUDA tensors ``sums`` (K, B, 3: sum e, sum e^2, sum a e), ``foot`` (K, 3: n, sum a, sum a^2), ``frame_corr``
    (K, B: Pearson of a and e_t), ``raw`` (K, B: the least-squares amplitude of a in e_t with a free offset), and, of every
    frame since the state was reset, ``image`` (K, vmax: the w-weighted mean of e_t over the box, x slowest, NaN past a box's
    n) and ``r_values`` (K: Pearson of a and the image) -- both None with ``finish=False``.  NaN where a variance is not
    positive or the weights sum to 0; an (k, t) whose box holds a sample that is not finite is NaN and has no part in the
    image.  A movie larger than one buffer goes in several calls with the same boxes and footprints, as in
    ``summary_images``: ``first=True`` resets ``state``, the last call has ``finish=True``; a later call may not be larger
    than the first.  float64 sums in a fixed order, no atomics: the same input gives the same bits.  ``segment``: frames per
    workgroup (0: the kernel's choice)."""
    fn = "component_stats"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows(fn, frames, sub, frame_ids, P)
    dev = frames.device
    K = _a_rows(fn, A_rows, P)
    for name, t in (("C", C), ("w", w)):
        _rows(t, fn, name, B, f" and rows of {B} floats")
        if t.dim() != 2 or t.shape[0] != K:
            raise ValueError(f"{fn}: {name} must be ({K}, {B}), got {tuple(t.shape)}")
    bh, bd, nvox = _boxes(fn, boxes, sz, K, dev=dev, check=False)     # the workspace entry below checks them
    lib = _lib.load()
    sz3 = _int3((X, Y, Z))
    need = _need(lib, "dnmf_component_stats_workspace", sz3, bh.data_ptr(), K, B, int(segment))
    # the boxes may change between the calls, and with them the bytes: the library judges a later call's state
    state = _stream_state(fn, state, need, first, dev, sized=False)
    vmax = int(nvox.max())
    f64 = dict(dtype=torch.float64, device=dev)
    sums, foot = torch.empty((K, B, 3), **f64), torch.empty((K, 3), **f64)
    frame_corr, raw = torch.empty((K, B), **f64), torch.empty((K, B), **f64)
    image = torch.empty((K, vmax), **f64) if finish else None
    r_values = torch.empty((K,), **f64) if finish else None
    with _timed("component_stats"):
        rc = lib.dnmf_component_stats(frames.data_ptr(), _ld(frames, P), _ptr(sub), 0 if sub is None else _ld(sub, P), _ptr(fid), sz3,
                                      B, A_rows.data_ptr(), _ld(A_rows, P), bh.data_ptr(), bd.data_ptr(), K, C.data_ptr(), _ld(C, B),
                                      w.data_ptr(), _ld(w, B), 1 if first else 0, 1 if finish else 0, int(segment), state.data_ptr(),
                                      _nbytes(state), sums.data_ptr(), foot.data_ptr(), frame_corr.data_ptr(), raw.data_ptr(),
                                      _ptr(image), vmax, _ptr(r_values), _stream())
    _lib.check(rc, "dnmf_component_stats")
    return dict(sums=sums, foot=foot, frame_corr=frame_corr, raw=raw, image=image, r_values=r_values), state


# ---- K26: merging duplicate components ---------------------------------------------------------------------------------------------
MERGE_MAX_K = 4096                                                   # component_pairs forms (K, K) masks of the boxes
PAIR_SUMS = ("saa", "n", "si", "sj", "sii", "sjj", "sij", "scc")     # the columns dnmf_component_pairs writes


def candidate_pairs(boxes):
    """(N, 2) int32 on the boxes' device: every (k, k) and every i < j whose inclusive boxes intersect, i ascending, then j."""
    b = torch.as_tensor(boxes).long()
    lo, hi = b[:, 0::2], b[:, 1::2]
    meet = ((lo[:, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[:, None, :])).all(2)
    return torch.nonzero(torch.triu(meet)).to(torch.int32).contiguous()      # nonzero's result may be column-major


def component_pairs(A_rows, sz, boxes, C, pairs=None):
    """K26.  The statistics of pairs of components, tests/merge_restatement.py (``pair_stats``) on the GPU.  ``A_rows`` (K, >= P)
    fp32 CUDA, the footprints as rows; ``boxes`` (K, 6) int32 inclusive boxes of at most 4096 voxels (``component_boxes``); ``C``
    (K, T) fp32 CUDA rows with unit inner stride, NaN allowed; ``pairs`` (N, 2) indices, i == j allowed -- None: every (k, k) and
    every i < j whose boxes intersect (``candidate_pairs``).  Returns a dict of CUDA tensors, float64 (N,) but ``pairs`` (N, 2)
    int32: ``saa`` = sum a_i a_j over the intersection of the boxes (0 where it is empty); over the frames where both traces are
    finite ``n``, their number, ``si``, ``sj``, ``sii``, ``sjj``, ``sij``, the sums of d_i, d_j, d_i^2, d_j^2 and d_i d_j with d = c
    - c[first such frame], and ``scc`` = sum c_i c_j; from them ``overlap`` = saa_ij / sqrt(saa_ii saa_jj) -- 0 where a norm is 0,
    NaN where (i, i) or (j, j) is not among the pairs -- and ``corr``, Pearson's from the shifted sums, NaN where n < 2 or a
    variance is not positive.  K <= 4096.  The boxes and the pairs are checked on the host before the launch: one synchronisation
    where they come from the GPU.  float64 sums in a fixed order, no atomics: the same input gives the same bits."""
    fn = "component_pairs"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    K = _a_rows(fn, A_rows, P)
    if K > MERGE_MAX_K:
        raise ValueError(f"{fn}: K={K} components, at most {MERGE_MAX_K}")
    dev = A_rows.device
    _rows(C, fn, "C")
    if C.dim() != 2 or C.shape[0] != K or C.device != dev:
        raise ValueError(f"{fn}: C must be ({K}, T) on {dev}, got {tuple(C.shape)} on {C.device}")
    T = C.shape[1]
    bh, bd, _ = _boxes(fn, boxes, sz, K, dev=dev, check=False)        # the library checks them, with the pairs
    ph = candidate_pairs(bh) if pairs is None else torch.as_tensor(pairs).detach()
    ph = ph.to("cpu", torch.int32).reshape(-1, 2).contiguous()
    pd = ph.to(dev)
    N = ph.shape[0]
    out = torch.empty((N, len(PAIR_SUMS)), dtype=torch.float64, device=dev)
    lib = _lib.load()
    with _timed("component_pairs"):
        rc = lib.dnmf_component_pairs(A_rows.data_ptr(), _ld(A_rows, P), _int3((X, Y, Z)), bh.data_ptr(), bd.data_ptr(), K,
                                      C.data_ptr(), _ld(C, T), T, ph.data_ptr(), pd.data_ptr(), N, out.data_ptr(), _stream())
    _lib.check(rc, "dnmf_component_pairs")
    st = {name: out[:, q] for q, name in enumerate(PAIR_SUMS)}
    pl = pd.long()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    diag = nan.repeat(K)
    on = pl[:, 0] == pl[:, 1]
    diag[pl[on, 0]] = st["saa"][on]
    den = diag[pl[:, 0]] * diag[pl[:, 1]]
    st["overlap"] = torch.where(den > 0, st["saa"] / torch.sqrt(den), torch.where(den == 0, torch.zeros_like(den), nan))
    n = st["n"]
    va, vb = n * st["sii"] - st["si"] * st["si"], n * st["sjj"] - st["sj"] * st["sj"]
    ok = (n >= 2) & (va > 0) & (vb > 0)
    st["corr"] = torch.where(ok, (n * st["sij"] - st["si"] * st["sj"]) / torch.sqrt(torch.where(ok, va * vb, torch.ones_like(va))), nan)
    st["pairs"] = pd
    return st


def _host64(stats):
    import numpy as np
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in stats.items()}


def merge_groups(stats, K, thr, min_overlap):
    """The groups of tests/merge_restatement.py (``groups_of``): the connected components of the edges ``corr >= thr and overlap
    >= min_overlap`` (NaN fails) among the pairs of ``stats`` (``component_pairs``), as a list of lists of indices -- members
    ascending, groups by their lowest member, so singletons keep their order.  On the host: a synchronisation."""
    s = _host64(stats)
    parent = list(range(int(K)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for (i, j), c, o in zip(s["pairs"].tolist(), s["corr"].tolist(), s["overlap"].tolist()):
        if i != j and c >= thr and o >= min_overlap:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    members = {}
    for k in range(int(K)):
        members.setdefault(find(k), []).append(k)
    return [members[r] for r in sorted(members)]


def merge_group_pairs(groups):
    """(N, 2) int32 CPU: every i <= j of every group of two members or more -- the pairs whose ``saa`` and ``scc`` are the S and
    Q of ``merge_plan``, whether or not the boxes intersect."""
    out = [(g[a], g[b]) for g in groups if len(g) >= 2 for a in range(len(g)) for b in range(a, len(g))]
    return torch.tensor(out, dtype=torch.int32).reshape(-1, 2)


def merge_plan(stats, K, thr, min_overlap, iters=10, group_stats=None):
    """Which components merge, and with which coefficients (tests/merge_restatement.py: ``plan``).  Float64 numpy on the host, a
    documented synchronisation: K is small, as in ``select_components``.  ``stats``: what ``component_pairs`` returned (the
    edges); ``group_stats``: a ``component_pairs`` result that lists every ``merge_group_pairs(groups)`` pair -- its ``saa`` and
    ``scc`` are the S and Q of the groups (None: ``stats`` itself, a ValueError where a pair is missing).  A group of m >= 2
    members becomes a' = sum u_k a_k, c' = sum w_k c_k, the rank-1 factor of sum_k a_k c_k^T in coefficient space: from u_k =
    sqrt(Q_kk), ``iters`` rounds of w = S u / (u^T S u), u = Q w / (w^T Q w); then u is scaled so that u^T S u = S_dd of the
    dominant member d (the largest sqrt(S_kk Q_kk)) and w inversely.  Returns a dict: ``groups`` (list of lists), ``offsets``
    (K' + 1) and ``members`` int32 (the CSR table of ``merge_apply``), ``u``, ``w`` and ``weight`` = sqrt(S_kk Q_kk) float64, one
    per member (1 for a singleton), ``dominant`` (K') int64 old indices, ``merged`` the number of groups with m >= 2."""
    import numpy as np
    groups = merge_groups(stats, K, thr, min_overlap)
    gs = _host64(stats if group_stats is None else group_stats)
    at = {(int(i), int(j)): p for p, (i, j) in enumerate(gs["pairs"].tolist())}

    def block(g, name):
        B = np.zeros((len(g), len(g)))
        for a in range(len(g)):
            for b in range(a, len(g)):
                p = at.get((g[a], g[b]), at.get((g[b], g[a])))
                if p is None:
                    raise ValueError(f"merge_plan: the pair ({g[a]}, {g[b]}) of the group {g} is not among the statistics "
                                     "(group_stats = component_pairs(..., pairs=merge_group_pairs(groups)))")
                B[a, b] = B[b, a] = gs[name][p]
        return B

    u_all, w_all, weight_all, dominant = [], [], [], []
    for g in groups:
        if len(g) == 1:
            u_all.append(np.ones(1)), w_all.append(np.ones(1)), weight_all.append(np.ones(1)), dominant.append(g[0])
            continue
        S, Q = block(g, "saa"), block(g, "scc")
        u = np.sqrt(np.diag(Q))
        w = np.zeros_like(u)
        for _ in range(int(iters)):
            w = S @ u / (u @ S @ u)
            u = Q @ w / (w @ Q @ w)
        weight = np.sqrt(np.diag(S) * np.diag(Q))
        d = int(np.argmax(weight))
        scale = np.sqrt(S[d, d] / (u @ S @ u))
        u, w = u * scale, w / scale
        if not (np.isfinite(u).all() and np.isfinite(w).all()):
            raise ValueError(f"merge_plan: the group {g} has no finite rank-1 factor (a footprint or a trace that is zero?)")
        u_all.append(u), w_all.append(w), weight_all.append(weight), dominant.append(g[d])
    sizes = [len(g) for g in groups]
    return dict(groups=groups, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                members=np.asarray([k for g in groups for k in g], dtype=np.int32), u=np.concatenate(u_all), w=np.concatenate(w_all),
                weight=np.concatenate(weight_all), dominant=np.asarray(dominant, dtype=np.int64), merged=sum(m >= 2 for m in sizes))


def merge_apply(A, C, plan, A_out=None, C_out=None):
    """K26.  The merged model of ``plan`` (``merge_plan``) in one launch: ``A`` (P, >= K) fp32 CUDA rows, the model's footprints
    with K fastest (``fp.A.reshape(P, K)``), ``C`` (K, >= T) fp32 CUDA rows -> ``(A_out (P, K'), C_out (K', T))`` fp32, A_out[v, g]
    = sum_k u_k A[v, k] and C_out[g, t] = sum_k w_k C[k, t] over the members of group g in their order, in float64, rounded once;
    a singleton with u = w = 1 comes out bit for bit.  ``A_out`` / ``C_out``: rows to write into (any row stride; floats past a
    row's extent are left alone), which may not overlap the inputs."""
    import numpy as np
    fn = "merge_apply"
    for name, t in (("A", A), ("C", C)):
        _rows(t, fn, name)
        if t.dim() != 2:
            raise ValueError(f"{fn}: {name} are rows, got {tuple(t.shape)}")
    P, K = A.shape
    T = C.shape[1]
    dev = A.device
    if C.shape[0] != K or C.device != dev:
        raise ValueError(f"{fn}: C must be ({K}, T) on {dev}, got {tuple(C.shape)} on {C.device}")
    off = torch.from_numpy(np.ascontiguousarray(plan["offsets"], dtype=np.int32))
    mem = torch.from_numpy(np.ascontiguousarray(plan["members"], dtype=np.int32))
    Kout = off.numel() - 1
    u = torch.from_numpy(np.ascontiguousarray(plan["u"], dtype=np.float64)).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(plan["w"], dtype=np.float64)).to(dev)
    if Kout < 1 or mem.numel() != int(off[-1]) or u.numel() != mem.numel() or w.numel() != mem.numel():
        raise ValueError(f"{fn}: the plan's offsets, members, u and w do not belong together")
    if A_out is None:
        A_out = torch.empty((P, Kout), dtype=torch.float32, device=dev)
    if C_out is None:
        C_out = torch.empty((Kout, T), dtype=torch.float32, device=dev)
    for name, t, shape in (("A_out", A_out, (P, Kout)), ("C_out", C_out, (Kout, T))):
        _rows(t, fn, name)
        if tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{fn}: {name} must be {shape} on {dev}, got {tuple(t.shape)} on {t.device}")
    od, md = off.to(dev), mem.to(dev)
    lib = _lib.load()
    with _timed("merge_apply"):
        rc = lib.dnmf_merge_apply(A.data_ptr(), _ld(A, K), P, K, C.data_ptr(), _ld(C, T), T, off.data_ptr(), mem.data_ptr(),
                                  od.data_ptr(), md.data_ptr(), Kout, u.data_ptr(), w.data_ptr(), A_out.data_ptr(), _ld(A_out, Kout),
                                  C_out.data_ptr(), _ld(C_out, T), _stream())
    _lib.check(rc, "dnmf_merge_apply")
    return A_out, C_out


# ---- K27: cleaning the footprints ---------------------------------------------------------------------------------------------------
CLEAN_METHODS = {"nrg": 0, "max": 1}              # the method and values arguments of dnmf_clean_footprints
CLEAN_VALUES = {"filtered": 0, "original": 1}
CLEAN_STATS = ("ok", "n_box", "n_cut", "n_closed", "n_parts", "n_kept")     # the int32 columns it writes


def clean_footprints(A, sz, boxes, method='nrg', nrgthr=0.9999, maxthr=0.2, median=True, closing=True, values='filtered', out=None):
    """K27.  Clean every footprint on its box, tests/footprint_clean_restatement.py on the GPU, bit for bit: the 3 x 3 x 3 median of
    the volume (``median``; 3 x 3 x 1 at Z = 1, coordinates clamped), the cut -- ``method='nrg'``: the largest values that hold
    ``nrgthr`` of the box's energy, every tie of the threshold kept; ``'max'``: the values above ``maxthr`` times the maximum --,
    the morphological closing by the full 3 x 3 x 3 element (``closing``), and of what is left the largest face-connected part
    by voxel count, a tie to the part with the lowest linear index.  On that part the result is the median (``values=
    'filtered'``) or the input (``'original'``), 0 on the rest of the column.  ``A`` (P, K) or (X, Y, Z, K) fp32 CUDA, K fastest;
    ``boxes`` (K, 6) int32 inclusive boxes of at most 4096 voxels (``component_boxes``), checked on the host before the launch:
    one synchronisation where they come from the GPU.  Returns ``(A_out, stats)``: ``A_out`` in the shape of ``A`` -- ``out``
    when given, which may be ``A`` itself -- and a dict of (K,) CUDA tensors: int32 ``ok``, ``n_box``, ``n_cut``, ``n_closed``,
    ``n_parts``, ``n_kept``, float64 ``threshold`` and ``energy`` (NaN for 'max').  A neuron whose box holds a negative or
    non-finite value or no positive one, or of which the cut keeps nothing, is refused, not deleted: ``ok = 0``, its column
    comes back bit for bit, its other counts are 0 and its threshold NaN.  No floating-point atomics and one sequential
    float64 sum: the same input gives the same bits."""
    fn = "clean_footprints"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    if method not in CLEAN_METHODS or values not in CLEAN_VALUES:
        raise ValueError(f"{fn}: method is one of {sorted(CLEAN_METHODS)} and values one of {sorted(CLEAN_VALUES)}, got {method!r} "
                         f"and {values!r}")
    if method == 'nrg' and not 0.0 < float(nrgthr) <= 1.0:
        raise ValueError(f"{fn}: nrgthr={nrgthr} outside (0, 1]")
    if method == 'max' and not float(maxthr) >= 0.0:
        raise ValueError(f"{fn}: maxthr={maxthr}, not >= 0")
    if not torch.is_tensor(A) or A.dim() not in (2, 4):
        raise ValueError(f"{fn}: A is a (P, K) or (X, Y, Z, K) tensor")
    _f32(A, f"{fn}: A")
    K = A.shape[-1]
    if K < 1 or A.numel() != P * K or (A.dim() == 4 and tuple(A.shape[:3]) != (X, Y, Z)):
        raise ValueError(f"{fn}: A must be ({P}, K) or ({X}, {Y}, {Z}, K), got {tuple(A.shape)}")
    dev = A.device
    bh, bd, _ = _boxes(fn, boxes, sz, K, noun="the box of neuron", dev=dev)
    if out is None:
        out = torch.empty_like(A)
    else:
        _f32(out, f"{fn}: out")
        if tuple(out.shape) != tuple(A.shape) or out.device != dev:
            raise ValueError(f"{fn}: out must be {tuple(A.shape)} on {dev}, got {tuple(out.shape)} on {out.device}")
    istats = torch.empty((K, len(CLEAN_STATS)), dtype=torch.int32, device=dev)
    dstats = torch.empty((K, 2), dtype=torch.float64, device=dev)
    lib = _lib.load()
    ws = _workspace(None, _need(lib, "dnmf_clean_footprints_workspace", K), dev)
    with _timed("clean_footprints"):
        rc = lib.dnmf_clean_footprints(A.data_ptr(), K, _int3((X, Y, Z)), bh.data_ptr(), bd.data_ptr(), K, CLEAN_METHODS[method],
                                       float(nrgthr), float(maxthr), 1 if median else 0, 1 if closing else 0, CLEAN_VALUES[values],
                                       out.data_ptr(), K, istats.data_ptr(), dstats.data_ptr(), ws.data_ptr(), _nbytes(ws), _stream())
    _lib.check(rc, "dnmf_clean_footprints")
    stats = {name: istats[:, q] for q, name in enumerate(CLEAN_STATS)}
    stats["threshold"], stats["energy"] = dstats[:, 0], dstats[:, 1]
    return out, stats


# ---- K28: new components from the residual -----------------------------------------------------------------------------------------
ADD_MAX_CANDIDATES = 4096      # the limits of dnmf_residual_boxes / dnmf_rank1_nmf; a box holds at most COMPONENT_MAX_VOXELS
ADD_MAX_FRAMES = 18432


def candidate_boxes(centres, sz, half):
    """(M, 6) int32 ``(x0, x1, y0, y1, z0, z1)``, inclusive, on the centres' device (the CPU for a list): per centre (M, 3) the voxel
    floor(centre + 0.5), moved into the volume, +- ``half`` voxels (one number or one per axis), cut to the volume -- the boxes
    ``residual_boxes`` takes."""
    X, Y, Z = (int(s) for s in sz)
    c = torch.as_tensor(centres).detach()
    if c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1:
        raise ValueError(f"candidate_boxes: centres must be (M, 3), got {tuple(c.shape)}")
    if not bool(torch.isfinite(c.double()).all()):
        raise ValueError("candidate_boxes: a centre is not finite")
    h = [int(half)] * 3 if isinstance(half, (int, float)) else [int(v) for v in half]
    if len(h) != 3 or min(h) < 0:
        raise ValueError(f"candidate_boxes: half={half!r} is one number >= 0 or one per axis")
    vox = torch.floor(c.double() + 0.5).long()
    boxes = torch.empty((c.shape[0], 6), dtype=torch.int32, device=c.device)
    for d, S in enumerate((X, Y, Z)):
        v = vox[:, d].clamp(0, S - 1)
        boxes[:, 2 * d] = (v - h[d]).clamp_min(0)
        boxes[:, 2 * d + 1] = (v + h[d]).clamp_max(S - 1)
    return boxes


def residual_boxes(frames, sz, boxes, sub=None, frame_ids=None, out=None, t0=0, n_total=None):
    """K28a.  The residual on candidate boxes -> ``E (M, n_total, vmax)`` fp32 CUDA: ``E[m, t0 + f, j] = frames_f(v_j) -
    sub_f(v_j)`` (one fp32 subtraction; the frame itself without ``sub``) for the voxels v_j of box m, x slowest as K24 numbers
    them; 0 for j past the box's voxels; a sample that is not finite is copied as it is.  ``frames`` (rows, ld >= P) fp32 CUDA
    rows in footprint coordinates, ``frame_ids``: the rows to take; ``sub`` (B, ld >= P): what the model predicts, row f for the
    f-th frame of the call; ``boxes`` (M, 6) int32 inclusive boxes inside the volume, of at most 4096 voxels
    (``candidate_boxes``).  A movie larger than one buffer goes in pieces: ``out`` = the E of the earlier calls, ``t0`` the first
    frame this call writes, ``n_total`` the frames of the movie (default: t0 + this call's); vmax = ``out.shape[2]``, else the
    largest box.  At most 4096 boxes and 18 432 frames."""
    fn = "residual_boxes"
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    fid, B = _frame_rows(fn, frames, sub, frame_ids, P)
    dev = frames.device
    bh, bd, nvox = _boxes(fn, boxes, sz, dev=dev)
    M, t0 = bh.shape[0], int(t0)
    if M > ADD_MAX_CANDIDATES:
        raise ValueError(f"{fn}: {M} candidates, at most {ADD_MAX_CANDIDATES}")
    n = t0 + B if n_total is None else int(n_total)
    if B < 1 or t0 < 0 or t0 + B > n:
        raise ValueError(f"{fn}: {B} frames at t0={t0} do not fit the {n} frames of E")
    if n > ADD_MAX_FRAMES:
        raise ValueError(f"{fn}: {n} frames, at most {ADD_MAX_FRAMES}")
    if out is None:
        out = torch.empty((M, n, int(nvox.max())), dtype=torch.float32, device=dev)
    else:
        _f32(out, f"{fn}: out")
        if out.dim() != 3 or tuple(out.shape[:2]) != (M, n) or out.shape[2] < int(nvox.max()) or out.device != dev:
            raise ValueError(f"{fn}: out must be ({M}, {n}, >= {int(nvox.max())}) on {dev}, got {tuple(out.shape)} on {out.device}")
    vmax = out.shape[2]
    if vmax > COMPONENT_MAX_VOXELS:
        raise ValueError(f"{fn}: vmax={vmax}, at most {COMPONENT_MAX_VOXELS}")
    lib = _lib.load()
    with _timed("residual_boxes"):
        rc = lib.dnmf_residual_boxes(frames.data_ptr(), _ld(frames, P), _ptr(sub), 0 if sub is None else _ld(sub, P), _ptr(fid),
                                     _int3((X, Y, Z)), B, bh.data_ptr(), bd.data_ptr(), M, out.data_ptr(), n, vmax, t0, _stream())
    _lib.check(rc, "dnmf_residual_boxes")
    return out


def rank1_nmf(E, nvox, a0, iters=5, workspace=None):
    """K28b.  Per candidate the non-negative rank-1 factor of its residual, tests/add_restatement.py (``rank1_nmf``) on the GPU.
    ``E`` (M, n, vmax) fp32 CUDA (``residual_boxes``), ``nvox`` (M,) the voxels of each box, ``a0`` (M, vmax) fp32 CUDA the start.
    Over the frames V whose ``nvox[m]`` samples are all finite, ``iters`` rounds of c_t = max(<a, e_t>, 0) / |a|^2 and a_j =
    max(sum_t c_t e_tj, 0) / |c|^2, then a scaled to |a0| and one more c-step.  Returns a dict of CUDA tensors: ``a`` (M, vmax)
    fp32, 0 past a box's voxels; ``c`` (M, n) fp32, NaN outside V; float64 ``energy`` = sum_{V, j} e^2, ``explained`` = 2 sum_t c_t
    <a, e_t> - |a|^2 |c|^2, ``saa`` = |a|^2 and ``scc`` = |c|^2 (M,); int32 ``n_valid`` and ``ok`` (M,).  A candidate whose |a|^2
    or |c|^2 becomes 0 or whose V is empty has ``ok = 0`` and NaN rows; nothing is raised.  float64 inside, sums in a fixed order,
    one rounding to fp32, no atomics: the same input gives the same bits.  vmax <= 4096, M <= 4096, n <= 18 432, iters >= 1."""
    fn = "rank1_nmf"
    _f32(E, f"{fn}: E")
    if E.dim() != 3:
        raise ValueError(f"{fn}: E must be (M, n, vmax), got {tuple(E.shape)}")
    M, n, vmax = E.shape
    dev = E.device
    if M < 1 or n < 1 or vmax < 1:
        raise ValueError(f"{fn}: E must be (M, n, vmax) with every extent >= 1, got {tuple(E.shape)}")
    if vmax > COMPONENT_MAX_VOXELS or M > ADD_MAX_CANDIDATES or n > ADD_MAX_FRAMES:
        raise ValueError(f"{fn}: E {tuple(E.shape)} above the limits ({ADD_MAX_CANDIDATES}, {ADD_MAX_FRAMES}, {COMPONENT_MAX_VOXELS})")
    if int(iters) < 1:
        raise ValueError(f"{fn}: iters={iters} must be at least 1")
    _f32(a0, f"{fn}: a0")
    if tuple(a0.shape) != (M, vmax) or a0.device != dev:
        raise ValueError(f"{fn}: a0 must be ({M}, {vmax}) on {dev}, got {tuple(a0.shape)} on {a0.device}")
    nh = torch.as_tensor(nvox).detach().to("cpu", torch.int32).reshape(-1)
    if nh.numel() != M or int(nh.min()) < 1 or int(nh.max()) > vmax:
        raise ValueError(f"{fn}: nvox must hold {M} counts in [1, {vmax}]")
    nd = nh.to(dev)
    lib = _lib.load()
    workspace = _workspace(workspace, _need(lib, "dnmf_rank1_nmf_workspace", M, n), dev)
    a = torch.empty((M, vmax), dtype=torch.float32, device=dev)
    c = torch.empty((M, n), dtype=torch.float32, device=dev)
    stats = torch.empty((M, 4), dtype=torch.float64, device=dev)
    info = torch.empty((2, M), dtype=torch.int32, device=dev)
    with _timed("rank1_nmf"):
        rc = lib.dnmf_rank1_nmf(E.data_ptr(), M, n, vmax, nd.data_ptr(), a0.data_ptr(), int(iters), a.data_ptr(), c.data_ptr(),
                                stats.data_ptr(), info[0].data_ptr(), info[1].data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                _stream())
    _lib.check(rc, "dnmf_rank1_nmf")
    return dict(a=a, c=c, energy=stats[:, 0], explained=stats[:, 1], saa=stats[:, 2], scc=stats[:, 3], n_valid=info[0], ok=info[1])


# ---- K29: the colours of a multi-channel model ------------------------------------------------------------------------------------
COLOUR_MAX_K, COLOUR_MAX_NC = 4096, 16          # the limits of dnmf_colour_normal_eqs / dnmf_colour_solve
COLOUR_LDS_MAX_K = 128                          # K29b holds M in LDS up to here and reads it from global memory beyond


def _colour_limits(fn, K, NC):
    if not (1 <= K <= COLOUR_MAX_K and 1 <= NC <= COLOUR_MAX_NC):
        raise ValueError(f"{fn}: K={K} neurons (1 .. {COLOUR_MAX_K}), NC={NC} channels (1 .. {COLOUR_MAX_NC})")


def _colour_system(fn, M, b, colours):
    """The checks of the two calls that read ``M`` (K, K), ``b`` (NC, K) float64 and ``colours`` (NC, K) fp32 -> (K, NC)."""
    _f32(colours, f"{fn}: colours")
    if colours.dim() != 2:
        raise ValueError(f"{fn}: colours must be (NC, K), got {tuple(colours.shape)}")
    NC, K = colours.shape
    _colour_limits(fn, K, NC)
    for name, t, shape in (("M", M, (K, K)), ("b", b, (NC, K))):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape and t.device == colours.device):
            raise ValueError(f"{fn}: {name} must be a contiguous float64 tensor {shape} on {colours.device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    return K, NC


def colour_normal_eqs(G, r, C, state=None, first=True, finish=True, out=None):
    """K29a.  The normal equations of the colours, tests/colours_restatement.py (``normal_eqs``) on the GPU -> ``(M, b, state)``.
    ``G`` (B, K, K) and ``r`` (NC, B, K) fp32 CUDA, contiguous: the Gram matrices of the UNCOLOURED warped footprints and their
    products with each channel of the B frames of the call; ``C`` (K, B) fp32 CUDA rows, the traces of those frames.  ``M`` (K, K)
    = sum_t G_t[k, l] C[k, t] C[l, t] and ``b`` (NC, K) = sum_t r_t^c[k] C[k, t], float64 CUDA (``out = (M, b)``: written there),
    over every frame since the state was reset -- both None with ``finish=False``.  A movie larger than one buffer goes in several
    calls, as in ``summary_images``: ``first=True`` resets ``state``, the last call has ``finish=True``; a later call may not be
    larger than the first.  The terms are formed in float64 and added in a fixed order that does not depend on the pieces: the
    same movie gives the same bits however it is cut.  No atomics.  K <= 4096, NC <= 16."""
    fn = "colour_normal_eqs"
    _f32(G, f"{fn}: G"), _f32(r, f"{fn}: r")
    if G.dim() != 3 or G.shape[1] != G.shape[2] or G.shape[0] < 1:
        raise ValueError(f"{fn}: G must be (B, K, K), got {tuple(G.shape)}")
    B, K, _ = G.shape
    if r.dim() != 3 or r.shape[1:] != (B, K) or r.device != G.device:
        raise ValueError(f"{fn}: r must be (NC, {B}, {K}) on {G.device}, got {tuple(r.shape)} on {r.device}")
    NC = r.shape[0]
    _colour_limits(fn, K, NC)
    _rows(C, fn, "C", B, f" and rows of {B} floats")
    if C.dim() != 2 or C.shape[0] != K or C.device != G.device:
        raise ValueError(f"{fn}: C must be ({K}, {B}) on {G.device}, got {tuple(C.shape)} on {C.device}")
    dev = G.device
    lib = _lib.load()
    state = _stream_state(fn, state, _need(lib, "dnmf_colour_normal_eqs_workspace", K, NC, B), first, dev)
    M = b = None
    if finish:
        if out is None:
            M = torch.empty((K, K), dtype=torch.float64, device=dev)
            b = torch.empty((NC, K), dtype=torch.float64, device=dev)
        else:
            M, b = out
            for name, t, shape in (("M", M, (K, K)), ("b", b, (NC, K))):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape and t.device == dev):
                    raise ValueError(f"{fn}: out {name} must be a contiguous float64 tensor {shape} on {dev}")
    with _timed("colour_normal_eqs"):
        rc = lib.dnmf_colour_normal_eqs(G.data_ptr(), r.data_ptr(), C.data_ptr(), _ld(C, B), K, NC, B, 1 if first else 0,
                                        1 if finish else 0, state.data_ptr(), _nbytes(state), _ptr(M), _ptr(b), _stream())
    _lib.check(rc, "dnmf_colour_normal_eqs")
    return M, b, state


def colour_solve(M, b, colours, sweeps=10):
    """K29b.  ``sweeps`` cyclic coordinate sweeps on ``1/2 x^T M x - b_c^T x, x >= 0`` per channel c from x = ``colours[c]``,
    tests/colours_restatement.py (``solve``) on the GPU.  ``M`` (K, K) and ``b`` (NC, K) float64 CUDA (``colour_normal_eqs``),
    ``colours`` (NC, K) fp32 CUDA, left as it is.  Returns a dict of CUDA tensors: ``colours`` (NC, K) fp32, a new tensor, x
    rounded once; ``kkt`` (NC) float64, the largest projected-gradient entry after the last sweep (zero at the solution); ``ok``
    (NC) int32, 0 for a channel whose ``b``, or ``M``, holds an entry that is not finite: it keeps its row and its kkt is NaN.
    A coordinate whose M[k, k] is not a positive finite number is left alone.  float64 inside, one workgroup per channel, M in
    LDS up to K = 128 and in global memory beyond; the same input gives the same bits.  K <= 4096, NC <= 16, sweeps >= 1."""
    fn = "colour_solve"
    K, NC = _colour_system(fn, M, b, colours)
    sweeps = _sweeps(fn, sweeps)
    dev = colours.device
    out = torch.empty((NC, K), dtype=torch.float32, device=dev)
    kkt = torch.empty((NC,), dtype=torch.float64, device=dev)
    ok = torch.empty((NC,), dtype=torch.int32, device=dev)
    with _timed("colour_solve"):
        rc = _lib.load().dnmf_colour_solve(M.data_ptr(), b.data_ptr(), colours.data_ptr(), K, NC, sweeps, out.data_ptr(),
                                           kkt.data_ptr(), ok.data_ptr(), _stream())
    _lib.check(rc, "dnmf_colour_solve")
    return dict(colours=out, kkt=kkt, ok=ok)


def colour_kkt(M, b, colours):
    """(NC) float64: the largest projected-gradient entry of ``1/2 x^T M x - b_c^T x, x >= 0`` at x = ``colours[c]`` (the measure
    ``colour_solve`` reports, for any colours); NaN for a channel whose ``b``, or ``M``, holds an entry that is not finite."""
    fn = "colour_kkt"
    K, NC = _colour_system(fn, M, b, colours)
    kkt = torch.empty((NC,), dtype=torch.float64, device=colours.device)
    ok = torch.empty((NC,), dtype=torch.int32, device=colours.device)
    with _timed("colour_kkt"):
        rc = _lib.load().dnmf_colour_solve(M.data_ptr(), b.data_ptr(), colours.data_ptr(), K, NC, 0, 0, kkt.data_ptr(),
                                           ok.data_ptr(), _stream())
    _lib.check(rc, "dnmf_colour_solve")
    return kkt


def pack_footprints_sparse(A, order):
    """A (..., K) and a neuron order -> (Aps (P,Ks), row_mask (P) uint8) for the zero-skipping Gram kernel."""
    K = A.shape[-1]
    A2 = _f32(A.reshape(-1, K), "A")
    lib = _lib.load()
    Ks = lib.dnmf_sparse_k(K)
    od = _i32(order, A.device)
    Aps = torch.empty((A2.shape[0], Ks), dtype=torch.float32, device=A.device)
    mask = torch.empty((A2.shape[0],), dtype=torch.uint8, device=A.device)
    _lib.check(lib.dnmf_pack_footprints_sparse(A2.data_ptr(), A2.shape[0], K, od.data_ptr(), Aps.data_ptr(), Ks,
                                               mask.data_ptr(), _stream()), "dnmf_pack_footprints_sparse")
    return Aps, mask


# when bench.py sets TIMING it also finds here the executed-work counters of the K3s launches (int64[2] tensor)
SPARSE_COUNTERS = None


# which zero-skipping kernel warp_gram_rhs_sparse runs: 'table' (local block table, 4 waves per SIMD) or 'static'
SPARSE_VARIANT = 'table'


def warp_gram_rhs_sparse(Aps, K, order, row_mask, sz, beta, times, frames, frame_ids=None, workspace=None, variant=None,
                         out=None):
    """K3s.  Returns G (B,K,K), r (B,K) in the original neuron order (written into the pair ``out`` when given)."""
    global SPARSE_COUNTERS
    lt = (variant or SPARSE_VARIANT) == 'table'
    X, Y, Z = (int(s) for s in sz)
    P = X * Y * Z
    dev = Aps.device
    _f32(Aps, "Aps"), _f32(beta, "beta")
    lib = _lib.load()
    od = _i32(order, dev)
    fid, tt, B = _ids(frames, frame_ids, times, dev)
    _rows(frames, "warp_gram_rhs_sparse", "frames")
    need = (lib.dnmf_warp_gram_rhs_sparse_lt_workspace if lt else lib.dnmf_warp_gram_rhs_sparse_workspace)(P, K, B)
    workspace = _workspace(workspace, need, dev)
    G, r = _gram_out(out, B, K, dev, "warp_gram_rhs_sparse")
    counters = None
    if TIMING is not None:
        if SPARSE_COUNTERS is None:
            SPARSE_COUNTERS = torch.zeros(2, dtype=torch.int64, device=dev)
        counters = SPARSE_COUNTERS
    with _timed("warp_gram_rhs_sparse"):
        rc = (lib.dnmf_warp_gram_rhs_sparse_lt if lt else lib.dnmf_warp_gram_rhs_sparse)(
            Aps.data_ptr(), Aps.shape[-1], K, od.data_ptr(), row_mask.data_ptr(), X, Y, Z, beta.data_ptr(),
            beta.shape[2], _ptr(tt), B, frames.data_ptr(), frames.stride(0), _ptr(fid), G.data_ptr(), r.data_ptr(),
            workspace.data_ptr(), _nbytes(workspace), _ptr(counters), _stream())
    _lib.check(rc, "dnmf_warp_gram_rhs_sparse")
    return G, r, workspace
