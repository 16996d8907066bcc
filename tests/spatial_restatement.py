"""Float64 definition of the sums of the dense footprint update K5 (``spatial_accum_kernel<NB>`` and ``trace_gram_kernel`` of
csrc/spatial_update.hip, reached through ``ops.spatial_accum`` and ``DeformableNMF._spatial_accum_dense``), the cases the
tests of K5 and of the dense K6 (``mu_spatial_kernel``, ``ops.mu_spatial``) share, and the bounds they hold every entry to.
numpy only; nothing here is fast.  K6 itself is ``hals_spatial_restatement.mu_spatial`` and is not restated here.

Definition.  A call names B frames: frame b is row ``fid_b`` of the frame buffer and column ``col_b`` of the traces,

    A1[p,k] = sum_b Y[fid_b, p] C[k, col_b]          S1[p,k] = sum_b |Y[fid_b, p]| |C[k, col_b]|
    Cs[k,l] = sum_b C[k, col_b] C[l, col_b]          Sc[k,l] = sum_b |C[k, col_b]| |C[l, col_b]|

with the rule of ``ops._ids`` (``index_rule``): ``times`` given -> B = len(times), col_b = times[b]; else ``frame_ids`` given ->
B = len(frame_ids), col_b = b; else B = every row of the buffer, col_b = b.  fid_b = frame_ids[b], or b without ``frame_ids``.
Rows, row padding and trace columns that no frame names are not part of the definition: the cases fill them with NaN.

Bounds.  u = 2^-24, the unit roundoff of fp32.  They follow from the arithmetic the kernels perform; no kernel output went into
them, and the ratios the GPU test measures are recorded there, apart from these.

  A1   The kernel sums the B products of an entry in fp32, four to an MFMA step, in an order of its own; an ``accumulate`` call
       adds its sum to what the buffer holds with one fp32 add.  A dot product of n terms summed in ANY order with every
       product and every add rounded once is off by at most gamma_n S, gamma_n = n u / (1 - n u) (Higham, Accuracy and
       Stability of Numerical Algorithms, (3.5)); ``pieces`` such sums with B terms in all, and ``pieces`` adds on top,
       give gamma_(B + pieces) S1.  What an MFMA step does inside (whether the four products of a step are rounded one by
       one or summed before one rounding) is not documented to the bit, so the bound is taken at twice the classical figure
       and two terms more:      |err| <= (B + pieces + 2) 2 u S1[p,k].
  Cs   The kernel sums in float64 (an error of B 2^-53 Sc, 2^-29 of u per term: nothing), rounds the sum of a piece to fp32
       once (u |sum| <= u Sc of the piece) and adds it to the buffer with one fp32 add (u |partial| <= u Sc); the first
       piece is added to 0, which is exact.  Over the pieces that is at most (2 pieces - 1) u Sc:
                                |err| <= 2 pieces u Sc[k,l].
       Entries (k,l) and (l,k) take the same products in the same order, so Cs equals its transpose bit for bit.
  K6   den = fmaf chain over l = 0 .. K-1 of a_l Cs[l,k] (K roundings, each at most u of the running sum of absolute values),
       then ``+ gamma D`` as a rounded product and a rounded add (the build does not contract), ``+ 1e-32f`` (one add), the
       product a_k A1 (one rounding) and an IEEE division (one).  With Dabs = sum_l |a_l| |Cs[l,k]| + |gamma| |D| + 1e-32 the
       denominator is off by at most (K + 3) u Dabs to first order, the quotient by that over |den| plus 2 u; again taken at
       twice the figure, and a little more:
                                |err| <= |want| 2 u ((K + 5) Dabs / |den| + 3),
       ``want`` the float64 result on the very fp32 A, A1, Cs, D the kernel gets and on float32(gamma).  First order means
       Dabs / |den| must stay small: the cases hold it at or below 4 wherever want != 0 (tests/test_spatial_restatement_host.py;
       the K6 inputs are non-negative, so it is 1).  A zero bound asks for an exact zero: a row of A = 0, an entry of A1 = 0.

Inputs (``values``): a fixed seed per case; magnitudes 2^e, e uniform in [-4, 2), rounded to fp32 (so within [2^-4, 4]: no
subnormals, MFMA denormal handling is not what this is about), signs at random for K5, about 10 % exact zeros.  One row of C
(not at K = 1) and one voxel of Y (not at P = 1) are all zero (their sums have a zero bound); the K6 inputs are non-negative,
one row of A is all zero (not at P = 1, where it would be the whole case) and A1 has its share of zeros.

K5 cases (``K5_CASES``; what each reaches is computed from its shape by ``geometry`` and asserted without a GPU in
tests/test_spatial_restatement_host.py).  The families nb, tail and voxels run in two layouts each: ``plain`` (rows of P floats,
no index lists) and ``idx`` (rows padded to a multiple of 4 floats so that full waves take the 16-byte loads, ``frame_ids`` a
permutation into a buffer of two spare rows, ``times`` another one into traces of three spare columns).
  nb-K        P 300, T 21, K in NB_K: the eight instantiations NB = (K+15)/16, each with a full and a ragged last block of 16
              (50 and 90 are added to the issue's list: without them NB = 4 and NB = 6 have no ragged block); P = 300 is one
              workgroup of four full waves and one wave of 44 voxels in a second workgroup
  tail-T      P 70, K 20, T in TAIL_T: an MFMA step of 4 frames, an iteration of 16, the prefetch one and two iterations past
              the end
  vox-P       K 20, T 21, P in VOX_P
  addr-P-...  (P, K, T) = (300, 33, 21) and (65, 33, 21): ldy = P, P+4, P+1, P+3; the base 1 float and 4 floats into the
              allocation (rows of a multiple of 4 floats, so that the base alone decides); frame_ids alone, times alone, both
  chan-P      P = 64 and 65: channel 1 of two-channel rows, ``rows[:, P:2P]`` -- ldy = 2 P, base P floats in (the dense form
              of MultiChannelDNMF); channel 0 is padding here and holds NaN
  big-K-...   P 70, T 21, K in (128, 129, 256) through ``DeformableNMF._spatial_accum_dense``: no lists, both lists, and
              frame_ids alone with two spare rows and three spare trace columns
K6 cases (``K6_CASES``): P in (1, 15, 16, 17, 33) x K in (1, 17, 100, 128, 129, 256) and (17, 1024), the last K the launcher
takes; each with D None, D and gamma 0.3, D and gamma 0 (``K6_MODES``)."""
import functools
import zlib

import numpy as np

import hals_spatial_restatement as HS
from gram_restatement import worst  # noqa: F401  (the tests take it from here)

F32 = np.float32
U = 2.0 ** -24

NB_K = (1, 15, 16, 17, 32, 33, 48, 50, 64, 65, 80, 90, 96, 100, 112, 127, 128)
TAIL_T = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)
VOX_P = (1, 3, 4, 63, 64, 65, 127, 128, 255, 256, 257, 320)
ADDR_SHAPES = ((300, 33, 21), (65, 33, 21))
BIG_K = (128, 129, 256)
K6_MODES = {"noD": (False, 0.0), "D-0.3": (True, 0.3), "D-0": (True, 0.0)}
K6_CASES = [(P, K) for K in (1, 17, 100, 128, 129, 256) for P in (1, 15, 16, 17, 33)] + [(17, 1024)]


def ceil4(n):
    return (n + 3) // 4 * 4


def _spec(P, K, T, ldy=None, offset=0, ids="none"):
    """``ids``: none | fid | times | both.  fid: two spare rows; times (and fid alone): three spare trace columns."""
    return {"P": P, "K": K, "T": T, "ldy": P if ldy is None else ldy, "offset": offset, "ids": ids}


def _both_layouts(stem, P, K, T):
    return {f"{stem}-plain": _spec(P, K, T), f"{stem}-idx": _spec(P, K, T, ldy=ceil4(P) + 4, ids="both")}


def _cases():
    out = {}
    for K in NB_K:
        out.update(_both_layouts(f"nb-{K}", 300, K, 21))
    for T in TAIL_T:
        out.update(_both_layouts(f"tail-{T}", 70, 20, T))
    for P in VOX_P:
        out.update(_both_layouts(f"vox-{P}", P, 20, 21))
    for P, K, T in ADDR_SHAPES:
        for pad in (0, 4, 1, 3):
            out[f"addr-{P}-ldy+{pad}"] = _spec(P, K, T, ldy=P + pad)
        for off in (1, 4):
            out[f"addr-{P}-base+{off}"] = _spec(P, K, T, ldy=ceil4(P), offset=off)
        for ids in ("fid", "times", "both"):
            out[f"addr-{P}-{ids}"] = _spec(P, K, T, ids=ids)
    for P in (64, 65):
        out[f"chan-{P}"] = _spec(P, 33, 21, ldy=2 * P, offset=P)
    for K in BIG_K:
        for ids in ("none", "both", "fid"):
            out[f"big-{K}-{ids}"] = _spec(70, K, 21, ids=ids)
    return out


K5_CASES = _cases()
SMALL = [n for n in K5_CASES if not n.startswith("big-")]           # what one launch of K5 takes through ops.spatial_accum
BIG = [n for n in K5_CASES if n.startswith("big-")]


def values(rng, shape, signed=True, zeros=0.1):
    """fp32: magnitudes 2^e, e uniform in [-4, 2); random signs when ``signed``; a share ``zeros`` of exact zeros."""
    v = np.exp2(rng.uniform(-4.0, 2.0, shape))
    if signed:
        v = v * rng.choice([-1.0, 1.0], shape)
    v[rng.random(shape) < zeros] = 0.0
    return v.astype(F32)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def index_rule(nrows, frame_ids, times):
    """(fid, col): the buffer row and the trace column of every frame of a call, by the rule of ``ops._ids``."""
    if times is not None:
        B = len(times)
        col = np.asarray(times, dtype=np.int64)
    else:
        B = len(frame_ids) if frame_ids is not None else int(nrows)
        col = np.arange(B)
    fid = np.asarray(frame_ids, dtype=np.int64)[:B] if frame_ids is not None else np.arange(B)
    return fid, col


def _permutation(rng, n, T, avoid=None):
    """T of 0 .. n-1 in a random order, not ascending where T allows it, and not ``avoid``."""
    for _ in range(100):
        p = rng.permutation(n)[:T]
        if (T < 2 or (np.diff(p) < 0).any()) and (avoid is None or not np.array_equal(p, avoid)):
            return p
    raise AssertionError("no permutation")


@functools.lru_cache(maxsize=None)
def k5_case(name):
    """The inputs of a case: dict(P, K, T, ldy, offset, ids, nrows, buf, C, frame_ids, times).  ``buf`` is the whole allocation
    (flat fp32): row r of the frame buffer is buf[offset + r ldy : offset + r ldy + P], everything else NaN.  ``C`` (K, columns)
    fp32, NaN in the columns no frame names.  frame_ids / times: int arrays or None.  Row 1 of C is all zero (not at K = 1,
    where it would be the whole case) and so is voxel P // 2 of every frame (not at P = 1)."""
    s = dict(K5_CASES[name])
    P, K, T, ldy, off = s["P"], s["K"], s["T"], s["ldy"], s["offset"]
    rng = _rng(name)
    spare_rows = 2 if s["ids"] in ("fid", "both") else 0
    spare_cols = 3 if s["ids"] != "none" else 0
    nrows = T + spare_rows
    fid = _permutation(rng, nrows, T) if spare_rows else None
    times = _permutation(rng, T + spare_cols, T, avoid=fid) if s["ids"] in ("times", "both") else None
    rows, cols = index_rule(nrows, fid, times)
    Y = values(rng, (T, P))
    if P > 1:
        Y[:, P // 2] = 0
    Cn = values(rng, (K, T))
    if K > 1:
        Cn[1] = 0
    buf = np.full(off + nrows * ldy, np.nan, dtype=F32)
    view = buf[off:].reshape(nrows, ldy)
    view[rows, :P] = Y
    C = np.full((K, T + spare_cols), np.nan, dtype=F32)
    C[:, cols] = Cn
    s.update(name=name, nrows=nrows, buf=buf, C=C, frame_ids=fid, times=times)
    return s


def frame_rows(c):
    """The (nrows, P) view of a case's frame buffer (numpy; the GPU test builds the same view of a device copy)."""
    return c["buf"][c["offset"]:].reshape(c["nrows"], c["ldy"])[:, :c["P"]]


def sums(Y, C, frame_ids=None, times=None):
    """The definition: Y (rows, P), C (K, columns) -> dict(A1, S1 (P,K), Cs, Sc (K,K), B) in float64."""
    fid, col = index_rule(Y.shape[0], frame_ids, times)
    y = np.asarray(Y)[fid].astype(np.float64)
    c = np.asarray(C)[:, col].astype(np.float64)
    return {"A1": y.T @ c.T, "S1": np.abs(y).T @ np.abs(c).T, "Cs": c @ c.T, "Sc": np.abs(c) @ np.abs(c).T, "B": len(fid)}


def tol_A1(ref, pieces=1):
    return (ref["B"] + pieces + 2) * 2 * U * ref["S1"]


def tol_Cs(ref, pieces=1):
    return 2 * pieces * U * ref["Sc"]


@functools.lru_cache(maxsize=None)
def k5_reference(name):
    """The float64 sums of a case, made once and left alone."""
    c = k5_case(name)
    return sums(frame_rows(c), c["C"], c["frame_ids"], c["times"])


def geometry(c):
    """What a launch of K5 on the case does, from its shape alone (csrc/spatial_update.hip): the instantiation NB and whether
    its last block of 16 traces is full; workgroups, waves, the waves whose 64 voxels lie inside P (``full_waves``) and
    how many of them take the 16-byte loads (all or none: ``wide_ok`` = base and row stride multiples of 16 bytes, the
    allocation itself being aligned), the voxels of the ragged wave; iterations of 16 frames, frames of the last one, frames of
    its last MFMA step; prefetches that lie wholly past the end (two are requested ahead of every iteration)."""
    P, K, T = c["P"], c["K"], c["T"]
    wide_ok = c["ldy"] % 4 == 0 and c["offset"] % 4 == 0
    iters = -(-T // 16)
    return {"nb": min((K + 15) // 16, 8), "full_block": K % 16 == 0, "workgroups": -(-P // 256), "waves": -(-P // 64),
            "full_waves": P // 64, "wide_ok": wide_ok, "wide_waves": P // 64 if wide_ok else 0, "ragged_voxels": P % 64,
            "iters": iters, "last_iter_frames": T - 16 * (iters - 1), "last_step_frames": (T - 1) % 4 + 1}


# ---- K6 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k6_case(P, K):
    """dict(A, A1, D (P,K), Cs (K,K)) fp32, non-negative; Cs is not symmetric (a transposed index would show)."""
    rng = _rng(f"k6-{P}-{K}")
    A, A1, D = (values(rng, (P, K), signed=False) for _ in range(3))
    if P > 1:
        A[P // 2] = 0
    return {"A": A, "A1": A1, "D": D, "Cs": values(rng, (K, K), signed=False)}


def k6_reference(A, A1, Cs, D, gamma):
    """(want, tol, ratio): the float64 K6 on these fp32 arrays and float32(gamma), its bound, and the largest Dabs / |den|
    over the entries with want != 0 (0 when there is none)."""
    g = float(F32(0.0 if gamma is None else gamma))
    A64, Cs64 = np.asarray(A, dtype=np.float64), np.asarray(Cs, dtype=np.float64)
    K = A64.shape[1]
    want = HS.mu_spatial(A64, A1, Cs64, D, g)
    den, dabs = A64 @ Cs64 + 1e-32, np.abs(A64) @ np.abs(Cs64) + 1e-32
    if D is not None:
        D64 = np.asarray(D, dtype=np.float64)
        den, dabs = den + g * D64, dabs + abs(g) * np.abs(D64)
    q = dabs / np.abs(den)
    live = want != 0
    return want, np.abs(want) * 2 * U * ((K + 5) * q + 3), float(q[live].max()) if live.any() else 0.0
