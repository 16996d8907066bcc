"""Float64 definition of K7 (``dnmf_image_iwarp``, csrc/image_iwarp.hip), the registered video: the warped position of every
voxel, the brute-force nearest-voxel search, and the warp families the tests hold the kernel's search certificate to.  numpy
only (``nearest64_torch`` is the same arithmetic on a torch tensor, for the GPU test); the case tables are shared by the host
test (tests/test_iwarp_restatement_host.py) and the GPU test (tests/test_gpu_iwarp_float64.py).  Nothing here is fast.

  positions64   Demix/dNMF.py:55, 81-83 in float64 on the fp32 coefficients: q = basis . beta, n = 2 q / (S - 1) - 1,
                s = ((n + 1) / 2) S.  Z = 1: n_z = -1 (the project's pin of the reference's 0 / 0), s_z = 0.  An axis of one voxel
                along x or y divides by zero like the reference: the position is inf or NaN there.
  nearest64     per lattice point the smallest (d2, voxel index), d2 = ((gx - sx)^2 + (gy - sy)^2) + (gz - sz)^2.  A d2 that
                is not finite counts as +inf: a lattice point without a finite distance takes voxel 0, which is what K7's
                exhaustive kernel returns (no comparison with a NaN or inf distance ever wins).
  margin        2 (2 sqrt(d2_min) delta + delta^2): how much larger than the float64 minimum the d2 (on positions64) of
                the voxel chosen on fp32 positions can be, when each of the two positions involved is off by at most delta.
                DELTA0 is the worst difference between positions64 and the oracle's fp32 ``pushforward_flow`` (measured by
                the host test on fixture G6 and two ``mixed`` warps of every shape of the table); DELTA = 4 DELTA0 covers the
                kernel's other fp32 order (the division shortcut, the fused multiply-adds).

The warp families (``warps``): every entry is an affine or quadratic map about the centre c = (S - 1) / 2 of the volume,
q(v) = c + t + A u + H [u_x^2, u_y^2, u_z^2, u_x u_y, u_x u_z, u_y u_z], u = v - c (``centred``).  At Z = 1 the z column is the
identity's.

Ties.  The reference scales by S, not S - 1, so under the identity voxel x sits at x S / (S - 1): for an even S the lattice
plane S / 2 lies exactly midway between the voxels S / 2 - 1 and S / 2 (at S = 2: the odd slice between both slices), and so it
does under every map that is symmetric about the centre along that axis or leaves the axis alone.  ``identity`` keeps those
ties -- it is the designed tie case, a share of 1 / X + 1 / Y (+ 1 / 2 at Z = 2) of the lattice points.  Every other entry carries
the extra shift TIE_BREAK (a few hundredths of a voxel, another value per axis), after which the two best distances of all but
a few lattice points differ by far more than NEAR_TIE = 1e-6 -- ``tie_share`` of the case is asserted below TIE_CAP by both tests.

``shift``.  Under a pure shift the nearest voxel of a lattice point that lost its pre-image is its projection onto the face of
the volume, which is a corner of the cell of the clamped pre-image: the box the kernel then searches certifies that corner
and never changes it, so a kernel without the box search passes every pure shift.  The entries of 0.5 and 3.7 voxels are
pure all the same (the box path must leave the cell's answer alone); the entries of 12.4 voxels ride on a rotation of 8
degrees about z (shifts along x, y) or on x gaining 0.3 z (shifts along z), which moves the nearest voxel 1.7 to 3.7 voxels
along the face, out of the cell -- they fail without the box.

``fold``.  A bare reflection is an isometry: the kernel's stretch bound (``min_stretch64``, the formula of
``iwarp_min_stretch``) is 0.98 for it at Z = 1 and 0.65 at Z > 1, and rightly so -- |s(a) - s(b)| >= m |a - b| holds.  It is kept
as the family ``mirror`` (the fixed-point walk of the search diverges under it: every lattice point away from the centre
needs a large box).  ``fold`` is the reflection with a bend along the reflected axis, x -> c - u + h u^2 with 2 h c_x = 2.4: the
determinant changes sign inside the volume, the bound is negative and every lattice point goes to the exhaustive kernel."""
import functools

import numpy as np

from oracle import dnmf_oracle as orc

F32 = np.float32
NEAR_TIE = 1e-6                # the project's bound between K7 / K10 / scipy: two best d2 closer than this are a tie
TIE_CAP = 0.01                 # largest share of such lattice points in a frame of any case but ``identity``
TIE_BREAK = (0.013, -0.021, 0.034)
DELTA0 = 8e-5                  # voxels; measured 6.6e-5 (test_positions64_against_the_oracle; at 20x300x1, |s| beyond 256)
DELTA = 4.0 * DELTA0
GIVE_UP = 1e-3                 # iwarp_stretch_kernel: a frame with m <= 1e-3 goes to the exhaustive kernel as a whole
CHUNK = 1 << 23                # distances held at once by the brute force (with its temporaries: below 64M doubles)

SHAPES = [(64, 64, 1), (20, 300, 1), (18, 70, 5), (33, 40, 2)]
THIN = [(1, 60, 3), (50, 1, 1), (40, 1, 4)]
FAMILIES = ("identity", "shift", "rotate", "zoom", "shear", "tilt", "bend", "nearfold", "fold", "mirror", "mixed")
THIN_FAMILIES = ("identity", "shift", "mixed")
MILD = {"identity": None, "rotate": (0,), "shear": None, "bend": (0,)}      # entries served without the fall-back (None: all)
PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]                    # rows 4..9 of beta


def cases():
    """Every (sz, family) the GPU test runs."""
    out = [(sz, k) for sz in SHAPES for k in FAMILIES if not (k == "tilt" and sz[2] == 1)]
    return out + [(sz, k) for sz in THIN for k in THIN_FAMILIES]


def case_id(c):
    return "x".join(map(str, c[0])) + "-" + c[1]


# ---- positions and the search ---------------------------------------------------------------------------------------------------
def lattice64(sz):
    return orc.voxel_lattice(sz).reshape(-1, 3).astype(np.float64)


def positions64(beta, sz):
    """(P, 3) float64: the warped position of every voxel, scaled by sz.  beta (10, 3), taken as fp32."""
    sz = tuple(int(s) for s in sz)
    b = np.asarray(beta, dtype=F32).astype(np.float64)
    v = lattice64(sz)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    basis = np.stack([np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z], 1)
    q = basis @ b
    out = np.empty_like(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        for d in range(3):
            if d == 2 and sz[2] == 1:
                out[:, d] = 0.0
                continue
            n = 2.0 * q[:, d] / (sz[d] - 1) - 1.0
            out[:, d] = ((n + 1.0) / 2.0) * sz[d]
    return out


def _d2(q, p, xp):
    d = ((q[:, None, 0] - p[None, :, 0]) ** 2 + (q[:, None, 1] - p[None, :, 1]) ** 2) + (q[:, None, 2] - p[None, :, 2]) ** 2
    return xp.where(xp.isfinite(d), d, xp.inf)


def nearest64(pts, lattice, chunk=CHUNK):
    """pts (N, 3), lattice (Q, 3) -> (index (Q,) int64, best d2 (Q,), second best d2 (Q,)), float64 brute force."""
    p = np.asarray(pts, dtype=np.float64)
    lat = np.asarray(lattice, dtype=np.float64)
    idx, best, second = np.empty(len(lat), np.int64), np.empty(len(lat)), np.full(len(lat), np.inf)
    rows = max(1, chunk // max(len(p), 1))
    for s in range(0, len(lat), rows):
        with np.errstate(invalid="ignore", over="ignore"):
            d = _d2(lat[s:s + rows], p, np)
        i = d.argmin(1)                                    # the first of the minima = the lowest index
        r = np.arange(len(i))
        idx[s:s + rows], best[s:s + rows] = i, d[r, i]
        if len(p) > 1:
            d[r, i] = np.inf
            second[s:s + rows] = d.min(1)
    return idx, best, second


def nearest64_torch(pts, lattice, chunk=CHUNK):
    """``nearest64`` on torch float64 tensors (any device): the same arithmetic, the lowest index by an explicit minimum."""
    import torch
    p, lat = pts.double(), lattice.double()
    N, Q = p.shape[0], lat.shape[0]
    idx = torch.empty(Q, dtype=torch.int64, device=p.device)
    best = torch.empty(Q, dtype=torch.float64, device=p.device)
    second = torch.full((Q,), float("inf"), dtype=torch.float64, device=p.device)
    ar = torch.arange(N, device=p.device)
    rows = max(1, chunk // max(N, 1))
    for s in range(0, Q, rows):
        d = _d2(lat[s:s + rows], p, torch)
        b = d.amin(1)
        i = torch.where(d == b[:, None], ar[None, :], N).amin(1)
        idx[s:s + rows], best[s:s + rows] = i, b
        if N > 1:
            d[torch.arange(len(i), device=p.device), i] = float("inf")
            second[s:s + rows] = d.amin(1)
    return idx, best, second


def chosen_d2(pts, lattice, chosen):
    """d2 between every lattice point and the voxel chosen for it (numpy or torch, float64); not finite counts as +inf."""
    xp = np if isinstance(pts, np.ndarray) else __import__("torch")
    e = lattice - pts[chosen]
    d = (e[:, 0] ** 2 + e[:, 1] ** 2) + e[:, 2] ** 2
    return xp.where(xp.isfinite(d), d, xp.inf)


def margin(best, delta=DELTA):
    return 2.0 * (2.0 * best ** 0.5 * delta + delta * delta)


def tie_share(best, second):
    """Share of lattice points whose two best d2 differ by less than NEAR_TIE (inf - inf: no tie)."""
    return float((second - best < NEAR_TIE).sum()) / max(len(best), 1)


# ---- the kernel's stretch bound -------------------------------------------------------------------------------------------------
def min_stretch64(beta, sz):
    """``iwarp_min_stretch`` of csrc/image_iwarp.hip in numpy: dict(m, smin, drift, det), det = the Jacobian determinant at
    the centre.  m <= GIVE_UP sends the frame to the exhaustive kernel."""
    b = np.asarray(beta, dtype=F32).astype(np.float64)
    X, Y, Z = (int(s) for s in sz)
    hz = Z > 1
    nd = 3 if hz else 2
    cx, cy, cz = 0.5 * (X - 1), 0.5 * (Y - 1), (0.5 * (Z - 1) if hz else 0.0)
    J = np.zeros((3, 3))
    hx = hy = hzz = 0.0
    for d in range(nd):
        b1, b2, b3, b4, b5, b6, b7, b8, b9 = b[1:, d]
        J[d] = [b1 + 2 * b4 * cx + b7 * cy + b8 * cz, b2 + 2 * b5 * cy + b7 * cx + b9 * cz, b3 + 2 * b6 * cz + b8 * cx + b9 * cy]
        if hz:
            hx += 4 * b4 * b4 + b7 * b7 + b8 * b8
            hy += b7 * b7 + 4 * b5 * b5 + b9 * b9
            hzz += b8 * b8 + b9 * b9 + 4 * b6 * b6
        else:
            hx += 4 * b4 * b4 + b7 * b7
            hy += b7 * b7 + 4 * b5 * b5
    Jn = J[:nd, :nd]
    off, fro = float(((Jn - np.eye(nd)) ** 2).sum()), float((Jn ** 2).sum())
    det = float(np.linalg.det(Jn))
    smin = 1.0 - np.sqrt(off)
    if hz:
        smin = max(smin, abs(det) / (0.5 * fro))
    else:
        disc = max(fro * fro - 4.0 * det * det, 0.0)
        smin = max(smin, np.sqrt(max(0.5 * (fro - np.sqrt(disc)), 0.0)) * (1.0 - 1e-9))
    drift = cx * np.sqrt(hx) + cy * np.sqrt(hy) + cz * np.sqrt(hzz)
    return {"m": 0.98 * (smin - drift), "smin": smin, "drift": drift, "det": det}


# ---- the warps ------------------------------------------------------------------------------------------------------------------
def centre(sz):
    return np.array([0.5 * (sz[0] - 1), 0.5 * (sz[1] - 1), 0.5 * (sz[2] - 1) if sz[2] > 1 else 0.0])


def centred(sz, A=None, t=None, H=None):
    """beta (10, 3) float64 of q(v) = c + t + A u + H [u_e u_f over PAIRS], u = v - c."""
    c = centre(sz)
    A = np.eye(3) if A is None else np.asarray(A, dtype=np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64)
    H = np.zeros((3, 6)) if H is None else np.asarray(H, dtype=np.float64)
    beta = np.zeros((10, 3))
    for d in range(3):
        beta[0, d] = c[d] + t[d] - A[d] @ c
        beta[1:4, d] = A[d]
        for j, (e, f) in enumerate(PAIRS):
            h = H[d, j]
            beta[4 + j, d] += h
            beta[1 + e, d] -= h * c[f]
            beta[1 + f, d] -= h * c[e]
            beta[0, d] += h * c[e] * c[f]
    if sz[2] == 1:
        beta[:, 2] = 0.0
        beta[3, 2] = 1.0
        beta[[3, 6, 8, 9], :2] = 0.0
    return beta


def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _flat(sz):
    """Axes the maps act on: z only for Z > 1."""
    return np.array([1.0, 1.0, 1.0 if sz[2] > 1 else 0.0])


def _bend_pattern(sz, rng=None):
    """A fixed (or drawn) H with a drift of 1 by the kernel's formula."""
    H = np.array([[0.9, -0.5, 0.4, 0.7, -0.3, 0.2], [-0.6, 0.8, -0.2, 0.5, 0.3, -0.4], [0.1, -0.2, 0.3, 0.15, -0.25, 0.2]])
    if rng is not None:
        H = rng.uniform(-1, 1, (3, 6))
    if sz[2] == 1:
        H[2] = 0.0
        H[:, [2, 4, 5]] = 0.0
    H[2] *= 0.1                                            # a volume is a few slices deep: bend z less
    return H / min_stretch64(centred(sz, H=H), sz)["drift"]


def warps(kind, sz, rng=None):
    """[(label, beta (10, 3) fp32)] of one family at one volume.  ``rng`` (numpy Generator) draws the ``mixed`` entries."""
    sz = tuple(int(s) for s in sz)
    hz = sz[2] > 1
    tb = np.array(TIE_BREAK) * _flat(sz)
    out = []

    def add(label, A=None, t=None, H=None, tie_break=True):
        t = (np.zeros(3) if t is None else np.asarray(t, dtype=np.float64)) + (tb if tie_break else 0.0)
        out.append((label, centred(sz, A, t, H).astype(F32)))

    if kind == "identity":
        out.append(("identity", orc.identity_beta(1)[:, :, 0]))
    elif kind == "shift":
        for amount in (0.5, 3.7, 12.4):
            for d in range(3 if hz else 2):
                for sign in (1.0, -1.0):
                    t = np.zeros(3)
                    t[d] = sign * amount
                    A = np.eye(3)
                    if amount > 10 and d < 2:
                        A = rot_z(8.0)
                    elif amount > 10:
                        A[0, 2] = 0.3
                    add(f"shift {'xyz'[d]}{sign * amount:+g}", A=A, t=t)
        add("shift all", t=np.array([2.3, -4.1, 1.6]) * _flat(sz))
    elif kind == "rotate":
        for deg in (2.0, 10.0, 30.0):
            add(f"rotate {deg:g}", A=rot_z(deg))
    elif kind == "zoom":
        add("zoom 0.7", A=np.diag([0.7, 0.7, 0.7 if hz else 1.0]))
        add("zoom 1.3", A=np.diag([1.3, 1.3, 1.3 if hz else 1.0]))
        add("zoom 0.8x1.25", A=np.diag([0.8, 1.25, 1.0]))
    elif kind == "shear":
        A = np.eye(3)
        A[0, 1] = 0.2
        add("shear", A=A)
    elif kind == "tilt":
        assert hz, "tilt needs Z > 1"
        A = np.eye(3)
        A[2, 0], A[2, 1], A[0, 2] = 0.02, -0.015, 0.3
        add("tilt", A=A)
    elif kind == "bend":
        H = _bend_pattern(sz)
        edge = 1.0 - GIVE_UP / 0.98                        # the drift at which m = GIVE_UP (smin = 1 at the centre)
        for drift in (0.05, 0.5, 0.999 * edge):
            add(f"bend {drift:.3g}", H=H * drift)
    elif kind == "nearfold":
        # x compressed by alpha ~ 1e-3 onto a thin band, tilted by 0.05 x per y so that it crosses lattice planes instead of
        # lying on one (the lattice points the band covers are near ties by construction: its voxels are 1e-3 apart); y and z
        # scaled by (S - 1) / S, which the reference's S / (S - 1) undoes: s_y = y + 0.005, s_z = z + 0.0085.  The lattice
        # points on the band are then within a few hundredths of a voxel of a warped one -- the only points a frame just
        # above the threshold still serves with a box (radius ~ 1000 (d0 + rho)); the box spans the volume along x.
        c, S = centre(sz), np.array(sz, dtype=np.float64)
        k = np.where(S > 1, (S - 1.0) / S, 1.0)
        o = 0.25 * np.abs(tb)
        t = o * k - c / S
        t[0] = (np.round(c[0] / k[0]) + 0.003) * k[0] - c[0]
        for label, target in (("nearfold above", 1.05 * GIVE_UP), ("nearfold below", 0.95 * GIVE_UP)):
            lo, hi = 0.0, 0.1
            for _ in range(60):                            # m grows with alpha
                A = np.array([[0.5 * (lo + hi), 0.05, 0.0], [0.0, k[1], 0.0], [0.0, 0.0, k[2] if hz else 1.0]])
                if min_stretch64(centred(sz, A, t).astype(F32), sz)["m"] < target:
                    lo = 0.5 * (lo + hi)
                else:
                    hi = 0.5 * (lo + hi)
            add(label, A=A, t=t, tie_break=False)
    elif kind == "fold":
        H = np.zeros((3, 6))
        H[0, 0] = 1.2 / max(centre(sz)[0], 1.0)
        add("fold", A=np.diag([-1.0, 1.0, 1.0]), H=H)
    elif kind == "mirror":
        add("mirror", A=np.diag([-1.0, 1.0, 1.0]))
    elif kind == "mixed":
        assert rng is not None, "mixed needs a generator"
        for i in range(3):
            A = rot_z(rng.uniform(-8, 8)) @ np.diag([rng.uniform(0.9, 1.12), rng.uniform(0.9, 1.12), 1.0])
            S = np.eye(3)
            S[0, 1], S[1, 0] = rng.uniform(-0.1, 0.1, 2)
            if hz:
                S[2, 0], S[2, 1], S[0, 2] = rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-0.2, 0.2)
            add(f"mixed {i}", A=A @ S, t=rng.uniform(-3, 3, 3) * _flat(sz), H=_bend_pattern(sz, rng) * 0.1)
    else:
        raise KeyError(kind)
    return out


def _seed(sz, kind):
    return int(np.random.SeedSequence([int(s) for s in sz] + [FAMILIES.index(kind)]).generate_state(1)[0])


@functools.lru_cache(maxsize=None)
def case(sz, kind):
    """(labels, beta (10, 3, B) fp32) of a family at a volume, the ``mixed`` entries from a seed of (sz, family)."""
    w = warps(kind, sz, np.random.default_rng(_seed(sz, kind)))
    return [l for l, _ in w], np.ascontiguousarray(np.stack([b for _, b in w], 2).astype(F32))


def is_mild(kind, i):
    return kind in MILD and (MILD[kind] is None or i in MILD[kind])


# ---- exact ties -----------------------------------------------------------------------------------------------------------------
TIE_SHAPES = [(17, 9, 2), (2, 17, 2), (33, 2, 1)]          # S - 1 a power of two on every axis: x S / (S - 1) is exact in fp32


def tie_case(sz):
    """(labels, beta (10, 3, B) fp32): the identity and integer-voxel shifts (no TIE_BREAK: the ties are the point)."""
    shifts = [(0, 0, 0), (1, 0, 0), (-2, 0, 0), (0, 3, 0), (0, -1, 0), (1, -2, 0)]
    if sz[2] > 1:
        shifts += [(0, 0, 1), (0, 0, -1), (-1, 2, 1)]
    betas = [centred(sz, t=np.array(t, dtype=np.float64)).astype(F32) for t in shifts]
    betas[0] = orc.identity_beta(1)[:, :, 0]
    return [f"shift {t}" for t in shifts], np.ascontiguousarray(np.stack(betas, 2))


# ---- more than 64 frames --------------------------------------------------------------------------------------------------------
MANY_SZ, MANY_B, MANY_FOLDS = (12, 10, 2), 70, (3, 66, 69)


def many_frames_case():
    """beta (10, 3, 70) fp32: frames 3, 66 and 69 ``fold``, the others the mild entries in turn."""
    mild = [case(MANY_SZ, k)[1][:, :, i] for k in MILD for i in range(case(MANY_SZ, k)[1].shape[2]) if is_mild(k, i)]
    fold = case(MANY_SZ, "fold")[1][:, :, 0]
    return np.ascontiguousarray(np.stack([fold if b in MANY_FOLDS else mild[b % len(mild)] for b in range(MANY_B)], 2))
