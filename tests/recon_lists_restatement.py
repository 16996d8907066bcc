"""Float64 definition of the list-form reconstruction image ``dnmf_recon_image_lists[_ex]`` (csrc/recon_lists.hip,
ops.recon_image_lists) and of the layout it reads (``dnmf_pack_footprints_lists``: At and bbox), for the very fp32 inputs the
kernels get.  numpy only, no torch and no GPU.  Also the case tables and their inputs, so that the host test
(tests/test_recon_lists_restatement_host.py) and the GPU test (tests/test_gpu_recon_lists_float64.py) speak of the same numbers.
Nothing here is fast.

The halo layout.  HALO = 2; a padded row holds rowf = ceil((Y + 4) Z / 32) 32 floats; voxel (x, y, z) sits at
(x + 2) rowf + (y + 2) Z + z; an image has Pp = (X + 4) rowf floats.  Everything that is not a voxel -- the border and the
floats of a row beyond (Y + 4) Z -- is zero.

The tile lists, from the geometry alone.  Padded row r holds volume row r - 2, and position u < (Y + 4) Z of the padded
(y, z) plane belongs to volume column floor(u / Z) - 2.  A tile is the padded rows 4 qx .. 4 qx + 3 and the positions
64 qu .. 64 qu + 63: it covers the volume rows 4 qx - 2 .. 4 qx + 1 and the volume columns floor(64 qu / Z) - 2 ..
floor(min(64 qu + 63, (Y + 4) Z - 1) / Z) - 2.  The list of a tile is every neuron with a non-empty box whose rows and whose
columns both meet the tile's, ascending (z is not looked at: a column lies in a tile with any of its z).  ``tile_member``
does not evaluate that formula: it marks the rows and the positions of every box and asks which tiles hold a mark.

The bound -- nothing in it comes from a kernel's output (U = 2^-24, the unit roundoff of fp32):
  |dS| <= n U sum_k |A[v,k] C[k,t]| (1 + n U) per entry, n the number of non-zero terms at that voxel and frame.  The kernel
  forms an entry as a chain of fmaf in ascending neuron index: one rounding per term, and a term with a zero factor adds an
  exact zero (so does a neuron that is listed without need).  A zero absolute sum demands an exact zero, which makes the
  border and the row excess part of the same comparison.
  One-hot traces and integers 0 .. 15 in both factors (sums below 2^24) do not round at all: bit equality.
Non-finite inputs are out of scope: the kernel drops terms by the boxes of the non-zeros, by design, so an infinite trace
times a zero footprint is a zero here and not a NaN."""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
HALO = 2
RL_NG = 8                                              # neurons a wave holds in registers at a time
EMPTY = (0x7fffffff, -1)                               # (lo, hi) per axis of an all-zero neuron, as the pack step leaves them
PATTERN = 7.0
FAMILIES = ("onehot", "integers", "random")
FAULTS = ("rim", "first8", "overwrite", "times", "z1", "zerobox")


def geometry(sz):
    X, Y, Z = (int(s) for s in sz)
    Xp, Yp = X + 2 * HALO, Y + 2 * HALO
    rowf = -(-(Yp * Z) // 32) * 32
    nu, nqx = -(-rowf // 64), -(-Xp // 4)
    return {"X": X, "Y": Y, "Z": Z, "P": X * Y * Z, "Xp": Xp, "Yp": Yp, "rowf": rowf, "Pp": Xp * rowf, "nu": nu, "nqx": nqx,
            "ntile": nqx * nu}


def halo_index(sz):
    """(P,) int64: the place of every voxel (x-major, then y, then z) in a halo-layout image."""
    g = geometry(sz)
    x, y, z = np.meshgrid(np.arange(g["X"]), np.arange(g["Y"]), np.arange(g["Z"]), indexing="ij")
    return ((x + HALO) * g["rowf"] + (y + HALO) * g["Z"] + z).reshape(-1)


def to_halo(V, sz):
    """(..., P) -> (..., Pp): the voxels in the halo layout, zero border and zero excess."""
    out = np.zeros(V.shape[:-1] + (geometry(sz)["Pp"],), dtype=V.dtype)
    out[..., halo_index(sz)] = V
    return out


def support_boxes(A, sz):
    """A (P, K) -> (K, 6) int64 [xlo, xhi, ylo, yhi, zlo, zhi], the inclusive bounding box of the non-zeros of each neuron
    (-0.0 is a zero).  An all-zero neuron keeps what the pack step initialises: lo = 0x7fffffff, hi = -1 on every axis."""
    g = geometry(sz)
    K = A.shape[1]
    nz = (np.asarray(A) != 0).reshape(g["X"], g["Y"], g["Z"], K)
    out = np.empty((K, 6), dtype=np.int64)
    for k in range(K):
        idx = np.nonzero(nz[..., k])
        for d in range(3):
            out[k, 2 * d], out[k, 2 * d + 1] = (idx[d].min(), idx[d].max()) if idx[d].size else EMPTY
    return out


def full_box(sz):
    g = geometry(sz)
    return (0, g["X"] - 1, 0, g["Y"] - 1, 0, g["Z"] - 1)


def tile_columns(sz, zmap=None):
    """(nu, 2): first and last volume column (may be border columns) that own a position of each run of 64 positions."""
    g = geometry(sz)
    u = np.arange(64 * g["nu"])
    col = np.where(u < g["Yp"] * g["Z"], u // (g["Z"] if zmap is None else zmap) - HALO, 10 ** 9).reshape(g["nu"], 64)
    return np.stack([col.min(1), np.where(col == 10 ** 9, -10 ** 9, col).max(1)], 1)


def tile_member(boxes, sz, zmap=None, want_rim=False):
    """(ntile, K) bool: neuron k's box meets tile qx nu + qu.  By marks: the padded rows and the positions of the padded plane
    that the box owns, then which groups of 4 rows and of 64 positions hold one.  ``zmap``: the Z of the position -> column map
    (the planted fault 'z1').  ``want_rim``: also (ntile, K) bool, the box reaches the tile by nothing but its first or its last
    row, or by nothing but its first or last column."""
    g = geometry(sz)
    b = np.asarray(boxes, dtype=np.int64)
    K = len(b)
    full = ((b[:, 0::2] <= b[:, 1::2]).all(1))[:, None]
    rows = np.arange(4 * g["nqx"]) - HALO
    rows = np.where(np.arange(4 * g["nqx"]) < g["Xp"], rows, 10 ** 9)[None, :]
    u = np.arange(64 * g["nu"])
    col = np.where(u < g["Yp"] * g["Z"], u // (g["Z"] if zmap is None else zmap) - HALO, 10 ** 9)[None, :]
    rowhit = (b[:, 0:1] <= rows) & (rows <= b[:, 1:2]) & full                         # (K, 4 nqx)
    colhit = (b[:, 2:3] <= col) & (col <= b[:, 3:4]) & full                           # (K, 64 nu)
    rt, ct = rowhit.reshape(K, g["nqx"], 4), colhit.reshape(K, g["nu"], 64)
    member = (rt.any(2)[:, :, None] & ct.any(2)[:, None, :]).reshape(K, -1).T
    if not want_rim:
        return member
    rowend = rowhit & ((rows == b[:, 0:1]) | (rows == b[:, 1:2]))
    rim_x = (rt.sum(2) == 1) & (rowend.reshape(K, g["nqx"], 4).sum(2) == 1)
    colr = np.broadcast_to(col, colhit.shape).reshape(K, g["nu"], 64)
    big = 10 ** 9
    cmin, cmax = np.where(ct, colr, big).min(2), np.where(ct, colr, -big).max(2)       # the columns of the overlap
    rim_y = ct.any(2) & (cmin == cmax) & ((cmin == b[:, 2:3]) | (cmin == b[:, 3:4]))
    rim = (rim_x[:, :, None] | rim_y[:, None, :]).reshape(K, -1).T
    return member, member & rim


def tile_lists(boxes, sz):
    """For every tile (qx nu + qu) the ascending list of the neurons whose box meets it."""
    return [np.flatnonzero(m) for m in tile_member(boxes, sz)]


def tile_of_position(sz):
    """(Pp,) int: the tile of every float of a halo image."""
    g = geometry(sz)
    r, u = np.divmod(np.arange(g["Pp"]), g["rowf"])
    return (r // 4) * g["nu"] + u // 64


def recon(A, C, times, sz):
    """(B, Pp) float64: S[b] = A . C[:, times[b]] in the halo layout, zero border and zero excess."""
    S = np.asarray(A, dtype=np.float64) @ np.asarray(C, dtype=np.float64)[:, list(times)]
    return to_halo(np.ascontiguousarray(S.T), sz)


def bound(A, C, times, sz):
    """(B, Pp) float64: n U sum_k |A[v,k] C[k,t]| (1 + n U) with n the non-zero terms of the entry; zero where there is none."""
    Ct = np.asarray(C)[:, list(times)]
    ab = np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(Ct.astype(np.float64))
    n = (np.asarray(A) != 0).astype(np.float64) @ (Ct != 0).astype(np.float64)
    return to_halo(np.ascontiguousarray((n * U * ab * (1.0 + n * U)).T), sz)


def worst(err, bnd):
    """(largest err / bound over bound > 0, its index, every zero-bound entry an exact zero)."""
    zero = bnd == 0
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bnd))
    idx = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    return (float(ratio.max()) if ratio.size else 0.0), idx, bool((err[zero] == 0).all())


def recon_tiled(A, C, times, sz, fault=None, preset=None):
    """The image as the kernel goes about it -- per tile the sum over the tile's list -- in float64, (B, Pp).  ``preset``: the
    call is one with skip_empty into rows that hold ``preset``: tiles with an empty list keep it.  ``fault`` plants one error:
      'rim'        a neuron is dropped from every tile that its box reaches only by its first or last row or column
      'first8'     only the first 8 neurons of a list are used
      'overwrite'  every group of 8 after the first overwrites the image instead of adding to it (the last group stays)
      'times'      frame b reads trace column b (mod T), not times[b]
      'z1'         the position -> column map of the tiles takes Z = 1
      'zerobox'    the box of an all-zero neuron counts as the full volume"""
    assert fault is None or fault in FAULTS
    g = geometry(sz)
    C = np.asarray(C, dtype=np.float64)
    boxes = support_boxes(A, sz)
    if fault == "zerobox":
        boxes[boxes[:, 0] > boxes[:, 1]] = full_box(sz)
    member, rim = tile_member(boxes, sz, zmap=1 if fault == "z1" else None, want_rim=True)
    if fault == "rim":
        member = member & ~rim
    rank, n = np.cumsum(member, 1) - 1, member.sum(1, keepdims=True)
    if fault == "first8":
        member = member & (rank < RL_NG)
    if fault == "overwrite":
        member = member & (rank // RL_NG == (n - 1) // RL_NG)
    tt = [b % C.shape[1] for b in range(len(times))] if fault == "times" else list(times)
    tid = tile_of_position(sz)
    W = to_halo(np.ascontiguousarray(np.asarray(A, dtype=np.float64).T), sz) * member[tid].T
    S = C[:, tt].T @ W
    if preset is not None:
        S[:, (member.sum(1) == 0)[tid]] = preset
    return S


def launch(sz, B):
    """The launch of dnmf_recon_image_lists_ex restated: frames per wave fpw = clamp(ceil(B ntile / 16384), 16, B), ny frame
    blocks of four waves, and the (block, wave) pairs whose first frame is past the end (they leave at once)."""
    ntile = geometry(sz)["ntile"]
    fpw = min(max(-(-(B * ntile) // 16384), 16), B)
    ny = -(-B // (4 * fpw))
    leave = {(by, w) for by in range(ny) for w in range(4) if (by * 4 + w) * fpw >= B}
    frames = {(by, w): min((by * 4 + w) * fpw + fpw, B) - (by * 4 + w) * fpw for by in range(ny) for w in range(4)
              if (by * 4 + w) * fpw < B}
    return {"fpw": fpw, "ny": ny, "leave": leave, "frames": frames}


def kernel_form(K):
    """NW of the instantiation (64 NW list slots a wave); None: refused."""
    return 1 if K <= 64 else 2 if K <= 128 else 4 if K <= 256 else None


# ---- the case tables ----------------------------------------------------------------------------------------------------------
# Nine volumes, the smallest that reach each edge: Z = 1, 2, 3, 5; X + 4 a multiple of 4 ((4,12,1), (8,60,1)) and not; rows that end on a tile
# ((8,60,1), (6,28,2): (Y + 4) Z = 64) and ragged ones ((9,20,3): 72 -> 96, (7,9,5): 65 -> 96, (41,130,1): 134 -> 160, three tiles).
# Two more, because at (9,20,3) and (7,9,5) the positions 63 | 64 lie in the last volume column and in the border: (5,30,3)
# (102 -> 128) and (6,20,5) (120 -> 128) have volume columns on both sides of them.
VOLUMES = [(1, 1, 1), (4, 12, 1), (8, 60, 1), (6, 28, 2), (5, 7, 3), (9, 20, 3), (7, 9, 5), (33, 31, 2), (41, 130, 1),
           (5, 30, 3), (6, 20, 5)]
FRAMES = [1, 15, 16, 17, 63, 64, 65, 70]
REFUSED_K = 257
LONG_CASE = {"sz": (5, 12, 2), "K": 20, "B": 349526, "T": 64}     # 3 tiles: B ntile = 1048578 > 64 * 16384, fpw 65
MODEL_K = (65, 129)
MODEL_SZ = (41, 130, 1)


def _seed(*parts):
    return int(np.random.SeedSequence([int(p) for p in parts]).generate_state(1)[0])


def edge_boxes(sz):
    """The boxes of an edge case, each with what it is there for: single voxels at the eight corners, an all-zero neuron, one
    that fills the volume; across every boundary between two runs of 64 positions four neurons -- one that ends on the last
    column before the next tile's first, one that ends on that first column, one that begins on the tile's last column, one
    that begins on the column after it (at Z | 64 the first and the last are the pair 63 | 64); across the padded rows 3 | 4
    and 7 | 8 (volume rows 1 | 2, 5 | 6) a neuron that ends on the one and a neuron that begins on the other."""
    g = geometry(sz)
    X, Y, Z = g["X"], g["Y"], g["Z"]
    boxes = [((x, x, y, y, z, z), "corner") for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
    boxes += [(None, "zero"), (full_box(sz), "full")]
    cols = tile_columns(sz)
    xs = (0, min(X - 1, 1))
    for qu in range(g["nu"] - 1):
        chi0, clo1 = int(cols[qu, 1]), int(cols[qu + 1, 0])
        for edge, ends, tag in ((clo1 - 1, True, "ends-before"), (clo1, True, "ends-on"), (chi0, False, "begins-on"),
                                (chi0 + 1, False, "begins-after")):
            if 0 <= edge <= Y - 1:
                ys = (max(0, edge - 2), edge) if ends else (edge, min(Y - 1, edge + 2))
                boxes.append((xs + ys + (0, Z - 1), f"{tag}-{qu}"))
    ys = (0, min(Y - 1, 2))
    for last in (1, 5):                                  # padded rows 3 | 4 and 7 | 8
        if X > last + 1:
            boxes.append(((last - 1, last) + ys + (0, Z - 1), f"xends-{last}"))
            boxes.append(((last + 1, min(X - 1, last + 2)) + ys + (0, Z - 1), f"xbegins-{last + 1}"))
    return boxes


def tile_interior(sz, qx, qu):
    """The volume rows and columns (inclusive, clipped to the volume) whose voxels lie in tile (qx, qu) ALONE."""
    g = geometry(sz)
    cols = tile_columns(sz)
    ylo = int(cols[qu, 0]) + (1 if qu > 0 and cols[qu - 1, 1] == cols[qu, 0] else 0)
    yhi = int(cols[qu, 1]) - (1 if qu + 1 < g["nu"] and cols[qu + 1, 0] == cols[qu, 1] else 0)
    return max(0, 4 * qx - HALO), min(g["X"] - 1, 4 * qx + 1), max(0, ylo), min(g["Y"] - 1, yhi)


STACKS = {(41, 130, 1): {(1, 0): 1, (2, 1): 8, (3, 2): 9, (5, 0): 16, (6, 1): 17, (8, 0): 25},
          (33, 31, 2): {(1, 0): 1, (2, 0): 8, (3, 0): 9, (4, 0): 16, (5, 0): 17, (7, 0): 26}}


def stack_boxes(sz):
    """Boxes stacked on single tiles (``STACKS``: tile -> how many), each inside its tile, in a shuffled neuron order, so that
    the lists have exactly these lengths and every other tile is empty; one neuron more is all zero."""
    rng = np.random.default_rng(_seed(*sz, 11))
    g = geometry(sz)
    boxes = []
    for (qx, qu), n in STACKS[sz].items():
        xlo, xhi, ylo, yhi = tile_interior(sz, qx, qu)
        for _ in range(n):
            x = np.sort(rng.integers(xlo, xhi + 1, 2))
            y = np.sort(rng.integers(ylo, yhi + 1, 2))
            boxes.append(((int(x[0]), int(x[1]), int(y[0]), int(y[1]), 0, g["Z"] - 1), f"stack-{qx}-{qu}"))
    boxes.append((None, "zero"))
    return [boxes[i] for i in rng.permutation(len(boxes))]


def random_boxes(sz, K, rng, ext=(4, 12)):
    """K boxes of up to ext[0] rows and ext[1] columns anywhere in the volume, every z."""
    g = geometry(sz)
    boxes = []
    for _ in range(K):
        x0, y0 = int(rng.integers(0, g["X"])), int(rng.integers(0, g["Y"]))
        boxes.append(((x0, min(g["X"] - 1, x0 + int(rng.integers(0, ext[0]))), y0, min(g["Y"] - 1, y0 + int(rng.integers(0, ext[1]))),
                       0, g["Z"] - 1), "random"))
    return boxes


def _k_boxes(sz, K):
    if (sz, K) == ((5, 7, 3), 256):
        return [(full_box(sz), "full")] * K                # every tile lists all 256: 32 groups of read-modify-write
    return random_boxes(sz, K, np.random.default_rng(_seed(*sz, K, 5)))


K_CASES = [((1, 1, 1), 1, 5), ((4, 12, 1), 1, 17), ((9, 20, 3), 64, 5), ((8, 60, 1), 64, 17), ((9, 20, 3), 65, 16), ((6, 28, 2), 65, 5),
           ((7, 9, 5), 128, 5), ((33, 31, 2), 128, 17), ((7, 9, 5), 129, 16), ((8, 60, 1), 129, 5), ((5, 7, 3), 256, 5),
           ((41, 130, 1), 256, 64)]

# name -> (sz, boxes with tags, B).  Every B at two volumes, every volume in an edge case.
CASES = {}
for _j in range(16):
    _sz, _B = VOLUMES[_j % len(VOLUMES)], FRAMES[_j % len(FRAMES)]
    CASES[f"edge-{'x'.join(map(str, _sz))}-B{_B}"] = (_sz, edge_boxes(_sz), _B)
for _sz, _B in (((41, 130, 1), 17), ((33, 31, 2), 3)):
    CASES[f"stack-{'x'.join(map(str, _sz))}-B{_B}"] = (_sz, stack_boxes(_sz), _B)
for _sz, _K, _B in K_CASES:
    CASES[f"K{_K}-{'x'.join(map(str, _sz))}-B{_B}"] = (_sz, _k_boxes(_sz, _K), _B)
EDGE_CASES = [n for n in CASES if n.startswith("edge")]
STACK_CASES = [n for n in CASES if n.startswith("stack")]
KFORM_CASES = [n for n in CASES if n.startswith("K")]
PACK_CASES = {sz: next(n for n in EDGE_CASES if CASES[n][0] == sz) for sz in VOLUMES}      # one pack check per volume


def case_boxes(name):
    """(K, 6) int64: the boxes the case places (an all-zero neuron: the empty box)."""
    return np.array([b if b is not None else EMPTY * 3 for b, _ in CASES[name][1]], dtype=np.int64)


def footprints(sz, boxes, family, rng):
    """A (P, K) fp32, dense and signed inside the boxes, zero outside.  integers: 0 .. 15; random: magnitudes in [0.25, 1] with
    exact zeros and -0.0 planted at about an eighth of the places; one-hot: the same without the zeros.  The two extreme corners
    of a box are never zero, so that the box of the non-zeros is the box that was placed."""
    g = geometry(sz)
    A = np.zeros((g["X"], g["Y"], g["Z"], len(boxes)), dtype=F32)
    for k, b in enumerate(boxes):
        if b is None:
            continue
        shape = (b[1] - b[0] + 1, b[3] - b[2] + 1, b[5] - b[4] + 1)
        if family == "integers":
            v = rng.integers(0, 16, shape).astype(F32)
        else:
            v = (rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(F32)
            if family == "random":
                m = rng.random(shape)
                v[m < 0.06] = 0.0
                v[(m >= 0.06) & (m < 0.12)] = -0.0
        for c in ((0, 0, 0), (-1, -1, -1)):
            if v[c] == 0:
                v[c] = 1.0
        A[b[0]:b[1] + 1, b[2]:b[3] + 1, b[4]:b[5] + 1, k] = v
    return A.reshape(-1, len(boxes))


def call_times(T, B, rng):
    """B columns out of T >= B + 1: a permutation, and with B >= 2 one repeat (the last names the first again)."""
    tt = rng.permutation(T)[:B]
    if B >= 2:
        tt[-1] = tt[0]
    return [int(t) for t in tt]


def make_inputs(sz, boxes, B, family, seed):
    """dict(A (P,K) fp32, C (K,T) fp32, calls: the ``times`` of every call, exact).  integers / random: one call, a permutation
    with one repeat out of T = B + 3 columns.  one-hot: T = K + 3 columns that each name one neuron, in a shuffled order; frame
    b of the call that starts at s names neuron (s + b) mod K, and there are as many calls of B frames as name every neuron."""
    rng = np.random.default_rng(seed)
    K = len(boxes)
    A = footprints(sz, boxes, family, rng)
    if family == "onehot":
        named = np.concatenate([rng.permutation(K), rng.integers(0, K, 3)])
        column_of = np.argsort(named[:K])
        C = np.zeros((K, K + 3), dtype=F32)
        C[named, np.arange(K + 3)] = 1.0
        calls = [[int(column_of[(s + b) % K]) for b in range(B)] for s in range(0, K, B)]
    else:
        if family == "integers":
            C = rng.integers(0, 16, (K, B + 3)).astype(F32)
            assert 15 * 15 * K < 2 ** 24
        else:
            C = (rng.uniform(0.25, 1.0, (K, B + 3)) * rng.choice([-1.0, 1.0], (K, B + 3))).astype(F32)
            C[rng.random(C.shape) < 0.05] = 0.0
        calls = [call_times(B + 3, B, rng)]
    return {"sz": sz, "A": A, "C": C, "calls": calls, "exact": family != "random", "family": family}


@functools.lru_cache(maxsize=8)
def case_inputs(name, family):
    sz, boxes, B = CASES[name]
    return make_inputs(sz, [b for b, _ in boxes], B, family, _seed(list(CASES).index(name), FAMILIES.index(family)))


def long_inputs():
    """The one case with fpw > 64 (``LONG_CASE``): integers, T = 64 trace columns named in a random order by B frames, so that
    there are only 64 different images.  dict(A, C, times (B,) int32, boxes)."""
    c = LONG_CASE
    rng = np.random.default_rng(_seed(*c["sz"], c["K"], 77))
    boxes = [b for b, _ in random_boxes(c["sz"], c["K"], rng, ext=(5, 12))]
    A = footprints(c["sz"], boxes, "integers", rng)
    C = rng.integers(0, 16, (c["K"], c["T"])).astype(F32)
    return {"A": A, "C": C, "times": rng.integers(0, c["T"], c["B"]).astype(np.int32), "boxes": boxes}


def model_inputs(K, family, B=9):
    """Compact footprints for ExponentialFP.recon_image at ``MODEL_SZ`` (well under six boxes a voxel): two sets of traces."""
    rng = np.random.default_rng(_seed(K, 31, family == "random"))
    boxes = [b for b, _ in random_boxes(MODEL_SZ, K, rng, ext=(5, 12))]
    a = make_inputs(MODEL_SZ, boxes, B, family, _seed(K, 32, family == "random"))
    a["C2"] = make_inputs(MODEL_SZ, boxes, B, family, _seed(K, 33, family == "random"))["C"]
    a["boxes"] = boxes
    return a
