"""Float64 definitions of the three dense forward kernels, for the very fp32 (render: float64) inputs the kernels get:
``dnmf_recon_image`` (csrc/recon_image.hip, the fp32-MFMA product S = A.C), K1 ``dnmf_warp_gather`` (csrc/warp_gather.hip, the
materialised A_t and grid) and ``dnmf_render_frames`` (csrc/render_frames.hip, the simulator's render loop).  numpy only; the
coordinates and the sample are gn_restatement's.  Also the case tables the tests share (``CASES_RECON``, ``CASES_K1``,
``CASES_RENDER``), their inputs and the bounds, so that the host test (tests/test_forward_restatement_host.py) and the GPU
test (tests/test_gpu_forward_float64.py) speak of the same numbers.  Nothing here is fast.

The bounds -- nothing in them comes from a kernel's output (U = 2^-24, the unit roundoff of fp32):

  recon, random signed inputs   |dS| <= (Kp + 1) U abs_sum per entry, abs_sum = |A| . |C|: every product and every addition
                                of a length-Kp fp32 dot product rounds at most once, in whatever order the matrix core takes
                                them; a zero abs_sum asks for an exact zero.  Kp = 16 ceil((K + 1) / 16).
  recon, one-hot / integers     bit equality: 1 a + 0 + .. + 0 and sums of integers below 2^24 do not round.
  recon by column groups        (ExponentialFP.recon_image at K > 127) the sum of the groups' bounds, plus U |running sum| for
                                every group added to the first (one fp32 addition each; the running sum is the exact one
                                plus what the bound so far lets it be off by).
  K1 A_t                        k2_restatement.recon_tol per channel: 4 spacing_fp32(max|u|) slope(A_k) + 1e-6 max|A_k|, the
                                project's bound for the same make_sample.  The zero-padded trilinear sample is continuous in
                                the coordinate: no flip condition for the value.
  K1 grid                       |dn_d| <= 13 U sum_a |phi_a| |2 beta_a| / (S_d - 1) + 2 U max(1, |n_d|): three monomial
                                products and ten fused steps, then one division and one subtraction.  Z = 1: n_z = -1 exactly.
  render                        |d| <= (K + 1) U sum_k |term_k|: the device exp may differ from numpy's in the last bit, which
                                moves a term by at most one fp32 step; each of the K partial sums may then round the other way."""
import functools
import time

import numpy as np

import gn_restatement as GN
import k2_restatement as K2R
from oracle import dnmf_oracle as orc

F32 = np.float32
U = 2.0 ** -24
HALO = 2


def padded_k(K):
    """Kp of the MFMA kernels: the channels rounded up to 16 with one spare column (asserted against ops.padded_k on the GPU)."""
    return 16 * -(-(int(K) + 1) // 16)


def worst(err, bound):
    """gram_restatement.worst: (largest err / bound over bound > 0, its index, every zero-bound entry an exact zero)."""
    zero = bound == 0
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    idx = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    return (float(ratio.max()) if ratio.size else 0.0), idx, bool((err[zero] == 0).all())


# ---- recon_image --------------------------------------------------------------------------------------------------------------
def recon(A, C, times):
    """(S, abs_sum), both (P, B) float64: S = A.reshape(P, K) . C[:, times], abs_sum = |A| . |C[:, times]|."""
    C = np.asarray(C)
    A2 = np.asarray(A).reshape(-1, C.shape[0]).astype(np.float64)
    Ct = C[:, list(times)].astype(np.float64)
    return A2 @ Ct, np.abs(A2) @ np.abs(Ct)


def recon_tol(K, abs_sum):
    return (padded_k(K) + 1) * U * abs_sum


GROUP = 112                                                # neurons per launch of ExponentialFP.recon_image at K > 127


def recon_grouped(A, C, times):
    """S and its bound for K > 127, summed by column groups of 112 as ExponentialFP.recon_image does: (S, bound) (P, B)."""
    K = np.asarray(C).shape[0]
    A2 = np.asarray(A).reshape(-1, K)
    S = bound = None
    for s0 in range(0, K, GROUP):
        cols = slice(s0, min(K, s0 + GROUP))
        part, ab = recon(A2[:, cols], np.asarray(C)[cols], times)
        tol = recon_tol(cols.stop - cols.start, ab)
        if S is None:
            S, bound = part, tol
        else:
            S = S + part
            bound = bound + tol
            bound = bound + U * (np.abs(S) + bound)
    return S, bound


RECON_VOLUMES = [(3, 5, 1), (4, 4, 1), (1, 17, 1), (32, 32, 1), (41, 25, 1), (9, 7, 5), (33, 31, 2), (65, 63, 1), (64, 64, 1),
                 (17, 241, 1)]
RECON_K = [1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127]
RECON_B = [1, 16, 17, 64, 65, 70]
# Every K at two volumes with ragged last voxel groups (P = 315 = 16 * 19 + 11, P = 1025 = 16 * 64 + 1) and two B, one on each
# side of 16 (NF = 1 | 4); every volume at two K and every B.  (sz, K, B) each.
SWEEP_K = {K: [((9, 7, 5), K, (1, 16)[i % 2]), ((41, 25, 1), K, (17, 65)[i % 2])] for i, K in enumerate(RECON_K)}
SWEEP_VOLUME = {sz: [(sz, K, B) for K in (RECON_K[(2 * i + 1) % 16], RECON_K[(2 * i + 8) % 16]) for B in RECON_B]
                for i, sz in enumerate(RECON_VOLUMES)}
CASES_RECON = [c for g in SWEEP_K.values() for c in g] + [c for g in SWEEP_VOLUME.values() for c in g]
FAMILIES = ("onehot", "integers", "random")
CHUNK_CASE = ((4, 4, 1), 3, 32770)                         # past the wrapper's 32768 frames a launch
GROUPED_K, GROUPED_SZ, GROUPED_B = (128, 130, 225), (33, 31, 2), (5, 20)   # groups 112 + 16, 112 + 18, 112 + 112 + 1


def _seed(*parts):
    return int(np.random.SeedSequence([int(p) for p in parts]).generate_state(1)[0])


def call_times(T, B, rng):
    """B columns out of T >= B + 1: a permutation, and with B >= 2 one repeat (the last names the first again)."""
    tt = rng.permutation(T)[:B]
    if B >= 2:
        tt[-1] = tt[0]
    return [int(t) for t in tt]


@functools.lru_cache(maxsize=8)
def recon_case(sz, K, B, family):
    """dict(A (P,K) fp32, C (K,T) fp32, calls: the ``times`` of every call, exact).  random / integers: one call of B
    frames, a permutation with one repeat out of T = B + 3 columns.  onehot: C[:, t] = e_t, T = K columns, as many calls of B
    (the last one wraps around) as name every column."""
    P = int(np.prod(sz))
    rng = np.random.default_rng(_seed(*sz, K, B, FAMILIES.index(family)))
    if family == "integers":
        A = rng.integers(0, 16, (P, K)).astype(F32)
        C = rng.integers(0, 16, (K, B + 3)).astype(F32)
        if K > 1:                                                  # first and last trace differ in every frame (B = 1 too)
            C[K - 1] = (C[0] + rng.integers(1, 16, B + 3)) % 16
        assert 15 * 15 * K < 2 ** 24
    else:
        A = rng.uniform(-1, 1, (P, K)).astype(F32)                 # dense and signed: this is the dense kernel
        C = rng.uniform(-1, 1, (K, B + 3)).astype(F32)
    if family == "onehot":
        C = np.eye(K, dtype=F32)
        order = rng.permutation(K)
        calls = [[int(order[(s + j) % K]) for j in range(B)] for s in range(0, K, B)]
    else:
        calls = [call_times(B + 3, B, rng)]
    return {"A": A, "C": C, "calls": calls, "exact": family != "random"}


def recon_wrong(A, C, times, K, which):
    """S of a deliberately wrong kernel (what the case must tell from the right one), on the padded operands: 'swap' two
    channels of A exchanged (the first and the last; at K = 1 the first and a padding column); 'slot' the channels of k-slot
    0, [0, Kp / 4), rotated by one; 'row' the last group of 16 voxels read one row early."""
    Kp = padded_k(K)
    Ap = np.zeros((A.shape[0], Kp))
    Ap[:, :K] = A
    Cp = np.zeros((Kp, len(times)))
    Cp[:K] = np.asarray(C, dtype=np.float64)[:, list(times)]
    if which == "swap":
        j = K - 1 if K > 1 else 1
        Ap[:, [0, j]] = Ap[:, [j, 0]]
    elif which == "slot":
        Ap[:, :Kp // 4] = np.roll(Ap[:, :Kp // 4], 1, axis=1)
    elif which == "row":
        p0 = (A.shape[0] - 1) // 16 * 16
        rows = np.arange(A.shape[0])
        rows[p0:] = np.maximum(rows[p0:] - 1, 0)
        Ap = Ap[rows]
    return Ap @ Cp


# ---- K1 -----------------------------------------------------------------------------------------------------------------------
CASES_K1 = list(K2R.SHAPES)
K1_ORDER = [3, 0, 5, 1, 6, 2, 4, 0]                         # frames F0 .. F6 of a call, not monotone; F0 is named twice
K1_REPEAT = (1, 7)                                          # the two places of F0


@functools.lru_cache(maxsize=None)
def k1_case(sz):
    """dict(A (X,Y,Z,5) fp32: k2_restatement.gaussians of sigma 3, some cut by the border; beta (10,3,8) fp32: case_betas with
    an extreme warp in the column no call names; times)."""
    sz = tuple(int(s) for s in sz)
    rng = np.random.default_rng(K2R.SEED.get(sz, 0))
    pos = np.stack([rng.uniform(-1, s, 5) for s in sz], 1)
    A = np.ascontiguousarray(np.moveaxis(K2R.gaussians(sz, pos, 3.0), 0, -1)).astype(F32)
    beta = K2R.case_betas(sz, rng).astype(np.float64)
    ext = np.zeros((10, 3))
    ext[0], ext[1, 0], ext[2, 1], ext[3, 2] = [1e5, -3e4, 7.0], -37.0, 0.01, 5.0
    beta[:, :, K2R.UNUSED] = ext
    return {"sz": sz, "A": A, "beta": beta.astype(F32), "times": [K2R.COL[i] for i in K1_ORDER]}


def warp_gather(A, beta, sz, times):
    """K1 in float64: dict(A_t (B,K,X,Y,Z), tol_A (B,K), grid (X,Y,Z,3,B), tol_grid (X,Y,Z,3,B)).  The coordinates are
    gn_restatement.source_coords (the reference's fp32 sequence), the blend gn_restatement.sample channel by channel; the grid
    is n_d = 2 q_d / (S_d - 1) - 1 in float64 from the fp32 coefficients (Z = 1: n_z = -1, bound 0)."""
    sz = tuple(int(s) for s in sz)
    A = np.asarray(A)
    K, B = A.shape[-1], len(times)
    beta = np.asarray(beta, dtype=F32)
    phi = GN.basis64(orc.voxel_lattice(sz))
    A_t, tol_A = np.zeros((B, K) + sz), np.zeros((B, K))
    grid, tol_g = np.zeros(sz + (3, B)), np.zeros(sz + (3, B))
    slope = [K2R.slope_of(A[..., k]) for k in range(K)]
    top = [float(np.abs(A[..., k]).max()) for k in range(K)]
    for b, t in enumerate(times):
        bt = beta[:, :, t]
        u = GN.source_coords(bt, sz)
        hit = np.ones(sz, bool)
        for d in range(3):
            hit &= (u[..., d] > -1) & (u[..., d] < sz[d])
        umax = float(np.abs(u[hit]).max()) if hit.any() else 0.0
        for k in range(K):
            A_t[b, k] = GN.sample(A[..., k].astype(np.float64), u)[0]
            tol_A[b, k] = 4.0 * float(np.spacing(F32(umax))) * slope[k] + 1e-6 * top[k]
        q2, a2 = phi @ (2.0 * bt.astype(np.float64)), np.abs(phi) @ np.abs(2.0 * bt.astype(np.float64))
        for d in range(3):
            if sz[d] == 1:
                grid[..., d, b], tol_g[..., d, b] = -1.0, 0.0
                continue
            n = q2[..., d] / (sz[d] - 1) - 1.0
            grid[..., d, b] = n
            tol_g[..., d, b] = 13 * U * a2[..., d] / (sz[d] - 1) + 2 * U * np.maximum(1.0, np.abs(n))
    return {"A_t": A_t, "tol_A": tol_A, "grid": grid, "tol_grid": tol_g}


@functools.lru_cache(maxsize=None)
def k1_reference(sz):
    """(result of ``warp_gather`` on ``k1_case(sz)``, host seconds), made once."""
    c = k1_case(sz)
    t0 = time.perf_counter()
    ref = warp_gather(c["A"], c["beta"], c["sz"], c["times"])
    return ref, time.perf_counter() - t0


# ---- render_frames --------------------------------------------------------------------------------------------------------------
RENDER_STD, RENDER_T = 3.0, 11
WINDOWS = [(0, None), (4, 3), (10, 1)]
BIG_FRAME, BIG_NEURON = 5, 1
CASES_RENDER = {f"{'x'.join(map(str, sz))}-K{K}-t{t0}": (sz, K, t0, T, 0.0)
                for sz in ((19, 23, 1), (9, 7, 5)) for K in (3, 300) for t0, T in WINDOWS}
CASES_RENDER["amp+1e30"] = ((19, 23, 1), 3, 0, None, 1e30)
CASES_RENDER["amp-1e30"] = ((19, 23, 1), 3, 0, None, -1e30)
RENDER_REFUSED_K = 2049


@functools.lru_cache(maxsize=None)
def render_case(name):
    """dict(sz, positions (K,3,11) fp32, traces (K,11) float64 in [0, 1], t0, T, shape_std).  Of every three neurons the first
    stays inside the volume, the second up to eight voxels outside it, the third jumps between inside and 10^4 voxels away
    from frame to frame.  ``amp``: neuron 1 (outside, 6.5 voxels before the first row) gets that amplitude in frame 5 -- voxels
    of the last rows are then 25 to 32 voxels from it, past the cut-off of an amplitude of 1 (r^2 < 629) and inside that of
    1e30 (r^2 < 1043), where its term is 1e-16 .. 1e-46 and every other term at least 10^10 times smaller."""
    sz, K, t0, T, amp = CASES_RENDER[name]
    rng = np.random.default_rng(_seed(*sz, K))
    ext = np.array(sz, dtype=np.float64)[None, :, None]
    pos = rng.uniform(0, 1, (K, 3, RENDER_T)) * (ext - 1)
    out = rng.uniform(1, 8, (K, 3, RENDER_T)) * rng.choice([-1.0, 1.0], (K, 3, RENDER_T))
    near = np.where(out < 0, out, ext - 1 + out)
    pos[1::3] = near[1::3]
    far = rng.uniform(0, 1, (K, 1, RENDER_T)) < 0.5
    pos[2::3] = np.where(far[2::3], pos[2::3] + 1e4 * rng.choice([-1.0, 1.0], (K, 3, RENDER_T))[2::3], pos[2::3])
    if sz[2] == 1:
        pos[:, 2] *= 0.01
    traces = rng.uniform(0, 1, (K, RENDER_T))
    if amp:
        pos[BIG_NEURON, :, BIG_FRAME] = [-6.5, 11.3, 0.0]
        pos[0, :, BIG_FRAME] = [4.2, 5.1, 0.0]
        pos[2, :, BIG_FRAME] = [1e4, -1e4, 0.0]
        traces[BIG_NEURON, BIG_FRAME] = amp
    return {"sz": sz, "positions": pos.astype(F32), "traces": traces, "t0": t0, "T": T, "shape_std": RENDER_STD}


def render(positions, traces, sz, shape_std, t0=0, T=None, order=None, r2_cut=None):
    """The kernel's own statement: per frame t0 .. t0 + T - 1 and voxel, amp_k exp(-r^2 / (2 shape_std)) in float64 (r^2 from
    the fp32 positions), cast to fp32, added in fp32 in neuron order.  Returns (video (T,P) fp32, abs_sum (T,P) float64 =
    sum_k |term_k| of the fp32 terms).  ``order``: the neurons to add, in that order (the wrong references of the host test);
    ``r2_cut``: terms at r^2 >= r2_cut are left out (the cut-off of a wrong amplitude)."""
    sz = tuple(int(s) for s in sz)
    K, _, T_total = positions.shape
    T = T_total - t0 if T is None else int(T)
    lat = orc.voxel_lattice(sz).astype(np.float64).reshape(-1, 3)
    video, abs_sum = np.zeros((T, len(lat)), dtype=F32), np.zeros((T, len(lat)))
    inv = 0.5 / float(shape_std)
    for k in (range(K) if order is None else order):
        c = positions[k, :, t0:t0 + T].astype(np.float64)                          # (3, T)
        d = lat[None, :, :] - c.T[:, None, :]
        r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        with np.errstate(under="ignore", over="ignore"):
            term = (np.asarray(traces, dtype=np.float64)[k, t0:t0 + T, None] * np.exp(-inv * r2)).astype(F32)
        if r2_cut is not None:
            term = np.where(r2 < r2_cut, term, F32(0))
        video = video + term
        abs_sum += np.abs(term.astype(np.float64))
    return video, abs_sum


def render_tol(K, abs_sum):
    return (K + 1) * U * abs_sum


def render_cut(shape_std, amp_max):
    """r2_cut of dnmf_render_frames for the amplitude it is told."""
    return 2.0 * shape_std * (np.log(max(amp_max, 1.0)) + 151.0 * 0.6931471805599453) + 1.0


@functools.lru_cache(maxsize=None)
def render_reference(name):
    """((video, abs_sum) of ``render`` on ``render_case(name)``, host seconds), made once."""
    c = render_case(name)
    t0 = time.perf_counter()
    ref = render(c["positions"], c["traces"], c["sz"], c["shape_std"], c["t0"], c["T"])
    return ref, time.perf_counter() - t0
