"""The Gram / rhs kernels K3 (ops.warp_gram_rhs), K3s (ops.warp_gram_rhs_sparse, 'table' and 'static') and K3n
(ops.warp_gram_rhs_lists) against the one float64 definition tests/gram_restatement.py, entry by entry.

Cases (gram_restatement.CASES; what each reaches is checked without a GPU in tests/test_gram_restatement_host.py):
  z1 (33, 257, 1) K 40      8 x 32 x 1 tiles, one-row and one-column ragged tiles, lists of 0 .. more than 8, staged and direct
  z1-dense-lists (33, 70, 1) K 12   every neuron listed nearly everywhere: groups of four, cross-group sums
  z2 (65, 300, 2) K 40      8 x 16 x 2 tiles, staged pairs, the long-list pass
  z3 (34, 90, 3) K 30       4 x 16 x 4 tiles with a ragged z tile, direct gathers only
  thin (9, 7, 5) K 3        one or two tiles, z taps outside on both sides
  words-64 | 65 | 128 | 129 | 256 (48, 64, 1)   one, two and four list words; K3 up to 65, K3s up to 128
  padK-15 | 16 | 17 | 127 (21, 19, 2)           K3's padded widths 16, 32, 32, 128 (every pattern fits K3n's 3800 slots)
  long (65537, 5, 1) K 4    FAST = 0 (IEEE division); a gross check: the coordinate term is most of the bound (printed)
  large-1 | 2 | 4 (2044, 2044, 1), (2044, 1020, 2), (2044, 508, 4) K 6, frames F5 and F0: halo images of exactly 2^24 bytes,
            F32OFF = false in all three Z forms; at B = 2 the plan is 64 chunks of 256 tiles: two passes chosen naturally
Frames F0 .. F6 are k2_restatement.case_betas', F7 scales x and y by 1.6 (no tile fits the staging region); a call takes them
in the order 3 0 7 5 1 6 2 4, so ``times`` is not monotone, out of a buffer of two spare rows with ldf = P + 8 through a
permuted ``frame_ids``; spare rows and padding hold other numbers, one column of beta holds an extreme warp no call names,
and G and r are preset to a non-zero pattern (an entry that is never written is seen).

Bound (gram_restatement.tol), per frame and entry:  2e-5 absG[k,l] + sum_v (|a_k| e_l + |a_l| e_k + e_k e_l) for G, 2e-5 absr[k]
+ sum_v |y| e_k for r, e_k(v) = 4 spacing_fp32(umax) L_k(v) + 1e-6 m_k(v); a zero bound asks for an exact zero.  K3n runs in
nine launch forms (passes auto | 1 | 2 times chunks auto | 1 | 3, the arguments of ops.warp_gram_rhs_lists: one wave per frame with runs of equal
lists; a ragged last chunk with list changes inside a run), each twice into one workspace (bit-identical) and each to the same
bound.  Between forms: K3s and K3n agree with K3 within the sum of their two bounds, entry by entry.
Slot-table route (warp_gram_rhs_lists(finish=False) + mu_temporal_slots, 7 rounds, gamma None, one case per Z form):
bit-equal to mu_temporal on the finished G, r; within one fp32 ulp of oracle.mu_temporal_from_gram on those fp32 G, r (the
K4 test's bound); and against the oracle on the FLOAT64 G, r at rtol 1e-4, the project's trace tolerance (header of
tests/test_gpu_parity.py) -- G and r each carry at most 2e-5 of a positive sum here (the route's frames are |y|, so r does
not cancel), one round C r / (G C) at most their sum 4e-5, and rounds do not add up because the update contracts towards its
fixed point.
Every test prints its worst |error| / bound and its host and GPU seconds.

Measured on the MI355X (kept apart from the bounds above, which they did not set): 19 cases, 41 tests, 8 s in all; the float64
references of the large volumes take 2.6 .. 2.9 s of host time each (two frames, footprint neighbourhoods only), every other
one under 2 s.  Largest |error| / bound, K3 = K3s table = K3s static to three digits | K3n over its nine forms:
  z1 0.068 | 0.068    z1-dense-lists 0.033 | 0.033    z2 0.032 | 0.032    z3 0.035 | 0.035    thin 0.0072 | 0.0042
  words-64 0.24 | 0.24    -65 0.13 | 0.13    -128 0.16 (K3s) | 0.17    -129 - | 0.15    -256 - | 0.21
  padK-15 0.053 | 0.053    -16 0.029 | 0.029    -17 0.037 | 0.034    -127 0.053 | 0.050
  long 0.012 | 0.012 (the coordinate term is 1.00 of the summed bound there: a gross check; 0.84 .. 0.99 in the other cases
  but thin 0.36 and z1-dense-lists 0.69 -- still 0.1 .. 1.5 % of a weak entry's own value, test_gram_restatement_host.py)
  large-1 0.0061 | 0.0041    large-2 0.0029 | 0.0022    large-4 0.013 | 0.0020
  K3 without a warp 0.011 / 0.017 / 0.013 of 2e-5 abs sum;  slot route 0.50 ulp, and 0.18 / 0.21 / 0.047 of rtol 1e-4.
The forms agree with each other far better than with float64: what is left is the shared sample (warp_taps.hpp) against the
reference's coordinate sequence, inside its allowance.  No kernel defect was found; c = 2e-5 was not raised."""
import functools
import time

import numpy as np
import pytest
import torch

import gram_restatement as GR
from test_gpu_mu_temporal import ulp_ratio

pytestmark = pytest.mark.gpu
F32 = np.float32
FORMS = [(p, c) for p in ("auto", "1", "2") for c in ("auto", "1", "3")]
DENSE = [n for n in GR.CASES if GR.CASES[n][1] <= 128]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


@pytest.fixture(scope="module")
def O():
    from oracle import dnmf_oracle
    return dnmf_oracle


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=1)
def device_inputs(name):
    """The case on the device: A (P,K); the frames in rows of a larger buffer addressed through frame_ids (spare rows and
    padding hold 5); beta; times.  One case at a time stays resident (the large ones take 0.5 GB with their layouts)."""
    c = GR.gram_case(name)
    B, P = c["frames"].shape
    rows = np.random.default_rng(7).permutation(B + 2)[:B]
    Fbuf = torch.full((B + 2, P + 8), 5.0, device="cuda")
    for b in range(B):
        Fbuf[int(rows[b]), :P] = dev(c["frames"][b])
    return {"A": dev(c["A"].reshape(P, c["K"])), "frames": Fbuf, "frame_ids": dev(rows, torch.int32), "beta": dev(c["beta"]),
            "times": dev(np.array(c["times"]), torch.int32)}


def preset(B, K):
    """(G, r) holding a non-zero pattern."""
    G = (torch.arange(B * K * K, device="cuda", dtype=torch.float32) % 5 + 3.25).reshape(B, K, K)
    r = -(torch.arange(B * K, device="cuda", dtype=torch.float32) % 3 + 1.5).reshape(B, K)
    return G, r


def check(name, what, G, r, ref):
    """Every entry of G (B,K,K), r (B,K) (fp32 numpy) within its bound, zero bounds as exact zeros, G symmetric bit for bit;
    returns the largest |error| / bound."""
    c = GR.gram_case(name)
    tG, tr = ref["tolG"], ref["tolr"]
    top = 0.0
    assert np.array_equal(G, G.transpose(0, 2, 1)), f"{name} {what}: G is not symmetric"
    for b, t in enumerate(c["times"]):
        for sym, got, want, bound in (("G", G[b], ref["G"][b], tG[b]), ("r", r[b], ref["r"][b], tr[b])):
            ratio, idx, zeros_ok = GR.worst(np.abs(got.astype(np.float64) - want), bound)
            where = f"{name} {what}: frame {b} (F{c['used'][b]}, column {t}) entry {sym}{list(idx)}"
            assert zeros_ok, f"{where[:where.index(' entry')]}: a {sym} entry with a zero bound is not an exact zero"
            assert ratio <= 1.0, f"{where}: |error| = {ratio:.3g} of the bound (value {want[idx]:.3g}, largest {np.abs(want).max():.3g})"
            top = max(top, ratio)
    return top


def with_tol(ref):
    tG, tr = GR.tol(ref)
    return {**ref, "tolG": tG, "tolr": tr}


def reference(name):
    ref, host = GR.reference(name)
    return with_tol(ref), host


def agree(name, what, G, r, G3, r3, ref):
    """Two kernel forms within the sum of their two bounds, entry by entry."""
    for b in range(len(G)):
        for sym, d, bound in (("G", np.abs(G[b].astype(np.float64) - G3[b]), 2 * ref["tolG"][b]),
                              ("r", np.abs(r[b].astype(np.float64) - r3[b]), 2 * ref["tolr"][b])):
            ratio, idx, zeros_ok = GR.worst(d, bound)
            assert zeros_ok and ratio <= 1.0, f"{name} {what} against K3: frame {b} entry {sym}{list(idx)}: {ratio:.3g} of the two bounds"


_k3 = {}


def k3(ops, name):
    """K3's G, r of a case (numpy), computed once: what K3s and K3n are compared with besides the float64 reference."""
    if name not in _k3:
        c, d = GR.gram_case(name), device_inputs(name)
        out = preset(len(c["times"]), c["K"])
        ops.warp_gram_rhs(ops.pack_footprints(d["A"]), c["K"], c["sz"], d["beta"], d["times"], d["frames"], frame_ids=d["frame_ids"],
                          out=out)
        _k3[name] = (out[0].cpu().numpy(), out[1].cpu().numpy())
    return _k3[name]


def test_large_volumes_are_past_the_offset_threshold(ops):
    """HaloLayout::f32off is ``halo bytes < 2^24``: the large shapes are on the far side of it, and just so; the others on the
    near side.  At their two frames the K3n plan has chunks of at least 100 tiles, so both passes are chosen without an
    override.  A change of the threshold, the layout or the plan then fails here instead of emptying the cases."""
    from dnmf_amd import _lib
    lib = _lib.load()
    for n in GR.LARGE:
        X, Y, Z = GR.CASES[n][0]
        assert ops.halo_voxels((X, Y, Z)) * 4 == 2 ** 24
        assert ops.halo_voxels((X - 1, Y, Z)) * 4 < 2 ** 24
        tx, ty, tz = GR.tile_shape((X, Y, Z))
        ntiles = -(-X // tx) * -(-Y // ty) * -(-Z // tz)
        chunk_len = -(-ntiles // 64)
        assert chunk_len >= 100 and lib.dnmf_warp_gram_rhs_lists_chunks(X, Y, Z, 2, 0, 0) == 2 * -(-ntiles // chunk_len)
    assert [GR.CASES[n][0][2] for n in GR.LARGE] == [1, 2, 4]
    for n in GR.SMALL:
        assert ops.halo_voxels(GR.CASES[n][0]) * 4 < 2 ** 24


@pytest.mark.parametrize("name", DENSE)
def test_dense_and_zero_skipping_forms(ops, name):
    """K3 (K <= 127) and both K3s variants (K <= 128) against float64, and K3s against K3."""
    c = GR.gram_case(name)
    sz, K, B = c["sz"], c["K"], len(c["times"])
    ref, host = reference(name)
    t0 = time.perf_counter()
    d = device_inputs(name)
    seen = {}
    if ops.padded_k(K) <= 128:
        G3, r3 = k3(ops, name)
        seen["K3"] = check(name, "K3", G3, r3, ref)
    order = np.random.default_rng(11).permutation(K).astype(np.int32)
    Aps, mask = ops.pack_footprints_sparse(d["A"], dev(order, torch.int32))
    for variant in ("table", "static"):
        out = preset(B, K)
        ops.warp_gram_rhs_sparse(Aps, K, dev(order, torch.int32), mask, sz, d["beta"], d["times"], d["frames"],
                                 frame_ids=d["frame_ids"], variant=variant, out=out)
        G, r = out[0].cpu().numpy(), out[1].cpu().numpy()
        seen["K3s " + variant] = check(name, "K3s " + variant, G, r, ref)
        if "K3" in seen:
            agree(name, "K3s " + variant, G, r, G3, r3, ref)
    gpu = time.perf_counter() - t0
    share = float(ref["coordG"].sum() / ref["tolG"].sum())
    print(f"\n{name}: |error| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in seen.items()) +
          f"; coordinate term {share:.2f} of the summed bound; host {host:.2f} s, GPU {gpu:.2f} s")


@pytest.mark.parametrize("name", list(GR.CASES))
def test_neuron_list_forms(ops, name):
    """K3n in its nine launch forms against float64, each twice into one workspace, and against K3 where K3 takes K."""
    c = GR.gram_case(name)
    sz, K, B = c["sz"], c["K"], len(c["times"])
    assert c["nslot"] <= GR.MAX_SLOTS          # every case's pattern fits K3n (padK-127 too at sigma 0.7)
    ref, host = reference(name)
    t0 = time.perf_counter()
    d = device_inputs(name)
    ly = ops.pack_footprints_lists(d["A"], sz)
    assert ly["nslot"] == c["nslot"] and np.array_equal(ly["bbox"].cpu().numpy()[c["bbox"][:, 0] <= c["bbox"][:, 1]],
                                                         c["bbox"][c["bbox"][:, 0] <= c["bbox"][:, 1]])
    G3 = r3 = None
    if ops.padded_k(K) <= 128:
        G3, r3 = k3(ops, name)
    seen, ws, tables = {}, None, set()
    from dnmf_amd import _lib
    for passes, chunks in FORMS:
        form = {"passes": 0 if passes == "auto" else int(passes), "chunks": 0 if chunks == "auto" else int(chunks)}
        tables.add(_lib.load().dnmf_warp_gram_rhs_lists_chunks(*sz, B, form["passes"], form["chunks"]))
        out = preset(B, K)
        _, _, ws = ops.warp_gram_rhs_lists(ly, K, sz, d["beta"], d["times"], d["frames"], frame_ids=d["frame_ids"], workspace=ws,
                                           out=out, **form)
        out2 = preset(B, K)
        _, _, ws2 = ops.warp_gram_rhs_lists(ly, K, sz, d["beta"], d["times"], d["frames"], frame_ids=d["frame_ids"], workspace=ws,
                                            out=out2, **form)
        assert ws2 is ws and torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1]), f"{name} passes {passes} chunks {chunks}"
        G, r = out[0].cpu().numpy(), out[1].cpu().numpy()
        what = f"K3n passes {passes} chunks {chunks}"
        seen[(passes, chunks)] = check(name, what, G, r, ref)
        if G3 is not None:
            agree(name, what, G, r, G3, r3, ref)
    gpu = time.perf_counter() - t0
    share = float(ref["coordG"].sum() / ref["tolG"].sum())
    print(f"\n{name}: K3n |error| / bound <= {max(seen.values()):.3g} over {len(seen)} forms (tables per frame {sorted(tables)}), "
          f"auto {seen[('auto', 'auto')]:.3g}; coordinate term {share:.2f} of the summed bound; host {host:.2f} s, GPU {gpu:.2f} s")


@pytest.mark.parametrize("name", ["z1", "z3", "padK-16"])
def test_no_warp(ops, name):
    """beta = None: every voxel takes its own footprint row with weight 1, so G = A^T A and r = A^T y of the unwarped fp32
    footprints, within the summation term 2e-5 absG / 2e-5 absr alone."""
    c = GR.gram_case(name)
    K, B = c["K"], len(c["times"])
    d = device_inputs(name)
    A = c["A"].reshape(-1, K).astype(np.float64)
    out = preset(B, K)
    ops.warp_gram_rhs(ops.pack_footprints(d["A"]), K, c["sz"], None, None, d["frames"], frame_ids=d["frame_ids"], out=out)
    G, r = out[0].cpu().numpy(), out[1].cpu().numpy()
    y = c["frames"].astype(np.float64)
    z = np.zeros((B, K, K))
    ref = {"G": np.broadcast_to(A.T @ A, (B, K, K)), "r": y @ A, "tolG": GR.C_SUM * np.broadcast_to(A.T @ A, (B, K, K)),
           "tolr": GR.C_SUM * (np.abs(y) @ A), "coordG": z}
    top = check(name, "K3 without a warp", G, r, ref)
    print(f"\n{name}: K3 without a warp, |error| / (2e-5 abs sum) <= {top:.3g}")


@pytest.mark.parametrize("name", ["z1", "z2", "z3"])
def test_slot_table_route(ops, O, name):
    """K3n's slot tables straight into K4 (no dense G in between), 7 rounds; the frames are |y| so that r is a positive sum."""
    c = GR.gram_case(name)
    sz, K, B = c["sz"], c["K"], len(c["times"])
    ref, _ = reference(name)
    d = device_inputs(name)
    ly = ops.pack_footprints_lists(d["A"], sz)
    assert ly["nbr"] is not None
    fr = d["frames"].abs()
    C0 = np.random.default_rng(5).uniform(0.5, 1.5, (K, B)).astype(F32)
    _, _, ws = ops.warp_gram_rhs_lists(ly, K, sz, d["beta"], d["times"], fr, frame_ids=d["frame_ids"], finish=False)
    Cs = ops.mu_temporal_slots(ly, ws, sz, dev(C0), 7)
    G, r, _ = ops.warp_gram_rhs_lists(ly, K, sz, d["beta"], d["times"], fr, frame_ids=d["frame_ids"])
    Cd = ops.mu_temporal(G, r, dev(C0), 7)
    assert torch.equal(Cs, Cd)
    got = Cs.cpu().numpy()
    same = O.mu_temporal_from_gram(np.moveaxis(G.cpu().numpy().astype(np.float64), 0, 2), r.cpu().numpy().astype(np.float64).T,
                                   C0, None, 7)
    ulps = ulp_ratio(got, same)
    want = O.mu_temporal_from_gram(np.moveaxis(ref["G"], 0, 2), ref["absr"].T, C0, None, 7)
    ratio, idx, zeros_ok = GR.worst(np.abs(got.astype(np.float64) - want), 1e-4 * np.abs(want))
    print(f"\n{name}: slot route {ulps:.3g} ulp from the oracle on the kernel's G, r; {ratio:.3g} of rtol 1e-4 from the oracle on "
          f"the float64 G, r (entry {idx})")
    assert ulps <= 1.0
    assert zeros_ok and ratio <= 1.0, f"{name}: trace {idx}: {ratio:.3g} of rtol 1e-4"
    assert (want > 0).sum() > 0.5 * want.size
