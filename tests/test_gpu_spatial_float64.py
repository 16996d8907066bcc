"""The dense footprint update -- K5 ``dnmf_spatial_accum`` (``spatial_accum_kernel<NB>``, ``trace_gram_kernel``) and K6
``dnmf_mu_spatial`` (``mu_spatial_kernel``) of csrc/spatial_update.hip, through ``ops.spatial_accum``, ``ops.mu_spatial``,
``DeformableNMF._spatial_accum_dense`` and ``DeformableNMF.update_spatial`` -- against the one float64 definition
tests/spatial_restatement.py, entry by entry.

Cases and bounds are that module's (its docstring derives the bounds; tests/test_spatial_restatement_host.py checks without a
GPU that every case reaches what it is named for):
  A1   |err| <= (B + pieces + 2) 2 u S1      Cs   |err| <= 2 pieces u Sc, and Cs == Cs^T bit for bit
  K6   |err| <= |want| 2 u ((K + 5) Dabs / |den| + 3)        u = 2^-24; a zero bound asks for an exact zero
Every K5 call writes into buffers preset to NaN (an entry that is never written is seen) and reads frames and traces whose
unnamed rows, padding and columns are NaN (a clamp that reaches unnamed data is seen); every call runs twice into fresh
buffers with the same bits.  Besides the cases: the 16-byte and the 4-byte load path on the same numbers (the allocation and
a copy one float further in) give the same bits; ``Ct`` NULL, ``Ct`` with rows of K and of K + 5 floats give the same bits
(the C ABI directly: ``ops`` always passes ``Ct``); 21 frames in pieces of 1, 16 and 4 through ``accumulate``; K = 128, 129
and 256 through ``_spatial_accum_dense`` in its three index forms against one reference; and ``update_spatial`` end to end
at (P, K, T) = (70, 129, 21), tolerance stated at the test.
Every test prints its worst |error| / bound and its host and GPU seconds.

Measured on the MI355X (kept apart from the bounds above, which they did not set): 159 tests, 3 s in all, the slowest 0.3 s
(the first launch); no float64 reference takes more than 0.02 s of host time.  Largest |error| / bound, A1 | Cs:
  nb plain 0.135 | 0.482, idx 0.124 | 0.481      tail plain 0.157 | 0.472, idx 0.154 | 0.495      vox plain 0.103 | 0.476, idx 0.082 | 0.475
  addr 0.092 | 0.487      chan 0.077 | 0.447      big (K 128, 129, 256) 0.110 | 0.483      three pieces 0.084 | 0.265
  K6 by K: 1 0.127, 17 0.088, 100 0.044, 128 0.040, 129 0.041, 256 0.031, 1024 0.014 (the three D modes within 1 % of each
  other)      update_spatial end to end 0.033
Cs sits just below one half: a single rounding of a float64 sum to fp32 is u |Cs|, the bound 2 u Sc.  A1 and K6 are random
walks of their roundings, far inside bounds that add them up in the worst case.  The load paths, the operand paths and
repeated runs agree bit for bit.  No kernel defect was found.  Two defects of the Python side were, and are fixed:
``ops.spatial_accum`` on a single trace column refused its own frame-major copy (the transpose of a (K, 1) tensor is
contiguous as it stands and keeps row stride 1 < K: tail-1-plain), and the K > 128 branch of ``_spatial_accum_dense`` took
C[:, :rows of the buffer] where the kernel takes C[:, :len(frame_ids)] (big-129-fid and big-256-fid came out NaN from the
spare columns).
Against scratch variants of the kernels (not kept): a tail mask of ``<= T`` fails every K5 case but tail-16, -32 and -48,
where the extra frame falls into an iteration the loop never runs (122 of the 128 tests that run K5, the K > 128 and
end-to-end ones among them); ``accumulate`` ignored in the A1 store fails the three-piece tests and nothing else; K6's
denominator loop stopping at K - 1 fails all 31 K6 cases and the end-to-end test."""
import time

import numpy as np
import pytest
import torch

import hals_spatial_restatement as HS
import spatial_restatement as SR

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd import _lib
    return _lib.load()


def dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def device_case(name, shift=0):
    """The case on the device: (Y, C, frame_ids, times) -- Y the (nrows, P) strided view of one allocation that holds the
    case's buffer ``shift`` floats in (0: as the case lays it out).  The allocation starts on a 16-byte boundary, which is what
    ``geometry`` assumes when it says which load path a wave takes."""
    c = SR.k5_case(name)
    flat = torch.full((shift + c["buf"].size,), float("nan"), device="cuda")
    flat[shift:] = dev(c["buf"])
    assert flat.data_ptr() % 16 == 0
    Y = torch.as_strided(flat, (c["nrows"], c["P"]), (c["ldy"], 1), storage_offset=shift + c["offset"])
    return Y, dev(c["C"]), dev(c["frame_ids"], torch.int32), dev(c["times"], torch.int32)


def nan_outputs(P, K):
    return torch.full((P, K), float("nan"), device="cuda"), torch.full((K, K), float("nan"), device="cuda")


def check(what, sym, got, want, bound):
    """Every entry of ``got`` (fp32 numpy) finite and within its bound of ``want``, zero bounds as exact zeros; a failure names
    the case, the entry, |error| / bound, the value and the largest value.  Returns the largest |error| / bound."""
    bad = np.argwhere(~np.isfinite(got))
    assert len(bad) == 0, f"{what}: entry {sym}{list(bad[0])} is {got[tuple(bad[0])]} ({len(bad)} of {got.size} entries not finite)"
    ratio, idx, zeros_ok = SR.worst(np.abs(got.astype(np.float64) - want), bound)
    assert zeros_ok, f"{what}: a {sym} entry with a zero bound is not an exact zero"
    assert ratio <= 1.0, (f"{what}: entry {sym}{list(idx)}: |error| = {ratio:.3g} of the bound (value {want[idx]:.3g}, "
                          f"largest {np.abs(want).max():.3g})")
    return ratio


def check_sums(what, A1, Cs, ref, pieces=1):
    """A1 and Cs (device tensors) of a case against its float64 sums -> (ratio of A1, ratio of Cs)."""
    a, c = A1.cpu().numpy(), Cs.cpu().numpy()
    r1 = check(what, "A1", a, ref["A1"], SR.tol_A1(ref, pieces))
    rc = check(what, "Cs", c, ref["Cs"], SR.tol_Cs(ref, pieces))
    assert np.array_equal(c, c.T), f"{what}: Cs is not symmetric bit for bit"
    return r1, rc


def timed_reference(name):
    t0 = time.perf_counter()
    ref = SR.k5_reference(name)
    return ref, time.perf_counter() - t0


@pytest.mark.parametrize("name", SR.SMALL)
def test_k5_cases(ops, name):
    """One launch of K5 per case through ``ops.spatial_accum``, ``accumulate=False`` into NaN, twice."""
    c = SR.k5_case(name)
    ref, host = timed_reference(name)
    t0 = time.perf_counter()
    Y, C, fid, tt = device_case(name)
    outs = []
    for _ in range(2):
        A1, Cs = nan_outputs(c["P"], c["K"])
        ops.spatial_accum(Y, C, frame_ids=fid, times=tt, A1=A1, Cs=Cs, accumulate=False)
        outs.append((A1, Cs))
    r1, rc = check_sums(name, *outs[0], ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"{name}: two runs differ"
    gpu = time.perf_counter() - t0
    print(f"\n{name}: |error| / bound A1 {r1:.3g}, Cs {rc:.3g}; host {host:.3f} s, GPU {gpu:.3f} s")


@pytest.mark.parametrize("name", ["addr-300-ldy+0", "addr-65-ldy+3", "chan-64", "nb-128-idx", "tail-49-idx"])
def test_wide_and_narrow_loads_give_the_same_bits(ops, name):
    """The same numbers where every full wave takes the 16-byte loads and, one float further into the allocation, where none
    can: the registers hold the same values and the MFMA sequence is the same, so A1 has the same bits."""
    c = SR.k5_case(name)
    g = SR.geometry(c)
    assert g["wide_ok"] and g["wide_waves"] >= 1
    t0 = time.perf_counter()
    got = []
    for shift in (0, 1):
        Y, C, fid, tt = device_case(name, shift)
        assert (Y.data_ptr() % 16 == 0) == (shift == 0) and Y.stride(0) % 4 == 0
        got.append(ops.spatial_accum(Y, C, frame_ids=fid, times=tt)[0])
    assert torch.equal(got[0], got[1]), f"{name}: the two load paths differ"
    r1 = check(name + " one float in", "A1", got[1].cpu().numpy(), SR.k5_reference(name)["A1"], SR.tol_A1(SR.k5_reference(name)))
    print(f"\n{name}: wide == narrow; |error| / bound A1 {r1:.3g}; GPU {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("name", ["addr-300-both", "addr-65-both", "nb-128-idx", "tail-17-plain"])
def test_trace_operand_paths_give_the_same_bits(lib, ops, name):
    """The C ABI directly: traces read neuron-major (``Ct`` NULL: the path ``ops`` never takes), frame-major with rows of K
    floats, and with rows of K + 5 floats whose padding is NaN."""
    c = SR.k5_case(name)
    P, K, T = c["P"], c["K"], c["T"]
    ref, host = timed_reference(name)
    t0 = time.perf_counter()
    Y, C, fid, tt = device_case(name)
    Ct = C.t().contiguous()
    Ctp = torch.full((C.shape[1], K + 5), float("nan"), device="cuda")
    Ctp[:, :K] = Ct
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for ct, ldct in ((None, 0), (Ct, K), (Ctp, K + 5)):
        A1, Cs = nan_outputs(P, K)
        rc = lib.dnmf_spatial_accum(Y.data_ptr(), Y.stride(0), ops._ptr(fid), C.data_ptr(), C.stride(0), ops._ptr(ct), ldct,
                                    ops._ptr(tt), T, P, K, A1.data_ptr(), Cs.data_ptr(), 0, stream)
        assert rc == 0, lib.dnmf_last_error()
        outs.append((A1, Cs))
    r1, rcs = check_sums(name + " Ct NULL", *outs[0], ref)
    for i, what in ((1, "ldct = K"), (2, "ldct = K + 5")):
        assert torch.equal(outs[0][0], outs[i][0]) and torch.equal(outs[0][1], outs[i][1]), f"{name}: Ct NULL and Ct with {what} differ"
    print(f"\n{name}: three operand paths agree; |error| / bound A1 {r1:.3g}, Cs {rcs:.3g}; host {host:.3f} s, "
          f"GPU {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("name", ["addr-300-both", "addr-65-both", "addr-300-ldy+0"])
def test_accumulate_in_three_pieces(ops, name):
    """21 frames as 1 + 16 + 4: the first piece with ``accumulate=False`` into NaN, the others added; the bounds with
    pieces = 3."""
    c = SR.k5_case(name)
    ref, host = timed_reference(name)
    t0 = time.perf_counter()
    Y, C, _, _ = device_case(name)
    fid, col = SR.index_rule(c["nrows"], c["frame_ids"], c["times"])
    A1, Cs = nan_outputs(c["P"], c["K"])
    for i, (a, b) in enumerate(((0, 1), (1, 17), (17, 21))):
        ops.spatial_accum(Y, C, frame_ids=[int(v) for v in fid[a:b]], times=[int(v) for v in col[a:b]], A1=A1, Cs=Cs,
                          accumulate=i > 0)
    r1, rc = check_sums(name + " in pieces of 1, 16, 4", A1, Cs, ref, pieces=3)
    print(f"\n{name}: three pieces, |error| / bound A1 {r1:.3g}, Cs {rc:.3g}; host {host:.3f} s, GPU {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("name", SR.BIG)
def test_more_than_128_neurons_by_column_groups(M, name):
    """``DeformableNMF._spatial_accum_dense`` at K = 128 (one launch), 129 and 256 (column groups of 128, C C^T in float64 by
    torch) in the three index forms: one index rule, one reference, the same bounds."""
    c = SR.k5_case(name)
    ref, host = timed_reference(name)
    t0 = time.perf_counter()
    Y, C, _, _ = device_case(name)
    lists = [None if v is None else [int(i) for i in v] for v in (c["frame_ids"], c["times"])]
    outs = []
    for _ in range(2):
        A1, Cs = nan_outputs(c["P"], c["K"])
        M.DeformableNMF._spatial_accum_dense(Y, C, A1, Cs, *lists)
        outs.append((A1, Cs))
    r1, rc = check_sums(name, *outs[0], ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"{name}: two runs differ"
    print(f"\n{name}: |error| / bound A1 {r1:.3g}, Cs {rc:.3g}; host {host:.3f} s, GPU {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("P,K", SR.K6_CASES)
def test_k6_cases(ops, P, K):
    """``ops.mu_spatial`` without D, with D and gamma 0.3, with D and gamma 0, each twice; a row of A = 0 and the entries of
    A1 = 0 have a zero bound."""
    c = SR.k6_case(P, K)
    d = {k: dev(v) for k, v in c.items()}
    seen, host, gpu = {}, 0.0, 0.0
    for mode, (withD, gamma) in SR.K6_MODES.items():
        t0 = time.perf_counter()
        want, tol, _ = SR.k6_reference(c["A"], c["A1"], c["Cs"], c["D"] if withD else None, gamma)
        t1 = time.perf_counter()
        got = [ops.mu_spatial(d["A"].clone(), d["A1"], d["Cs"], d["D"] if withD else None, gamma) for _ in range(2)]
        assert torch.equal(got[0], got[1]), f"K6 P {P} K {K} {mode}: two runs differ"
        seen[mode] = check(f"K6 P {P} K {K} {mode}", "A", got[0].cpu().numpy(), want, tol)
        host, gpu = host + t1 - t0, gpu + time.perf_counter() - t1
    print(f"\nK6 P {P} K {K}: |error| / bound " + ", ".join(f"{m} {r:.3g}" for m, r in seen.items()) +
          f"; host {host:.3f} s, GPU {gpu:.3f} s")


def test_update_spatial_end_to_end(M):
    """``DeformableNMF.update_spatial`` (numpy in, K5 by column groups, K6, float64 numpy out) at (P, K, T) = (70, 129, 21)
    against the restatement on float64 sums.  To first order the result a A1 / den moves by |a| dA1 / |den| when A1 moves by
    dA1, and K6 adds its own rounding, so

        tol = |A| tol_A1 / |den|  +  |want| 2 u ((K + 5) Dabs / |den| + 3)

    (the A1 bound carried through K6, plus the K6 bound).  C C^T comes out of a float64 product rounded once to fp32: u of
    every term of the denominator, non-negative here, so u of ``den`` itself -- inside the K6 bound, which counts K + 3
    roundings of that size and is taken twice.  Footprints, traces and D are non-negative (Dabs = den), the frames signed."""
    P, K, T, gamma = 70, 129, 21, 0.3
    rng = np.random.default_rng(70129)
    A, D = (SR.values(rng, (P, K), signed=False) for _ in range(2))
    A[P // 2] = 0
    C = SR.values(rng, (K, T), signed=False)
    Yi = SR.values(rng, (P, T))
    Yi[3] = 0
    t0 = time.perf_counter()
    ref = SR.sums(Yi.T, C)
    g = float(F32(gamma))
    want = HS.mu_spatial(A, ref["A1"], ref["Cs"], D, g)
    A64 = A.astype(np.float64)
    den = A64 @ ref["Cs"] + g * D.astype(np.float64) + 1e-32
    q = den / np.abs(den)                                     # Dabs / |den|: every term is non-negative
    assert (den > 0).all() and (q <= 4).all()
    tol = A64 * SR.tol_A1(ref) / den + np.abs(want) * 2 * SR.U * ((K + 5) * q + 3)
    t1 = time.perf_counter()
    got = M.DeformableNMF.update_spatial(A, C, Yi, D=D, gamma=gamma)
    assert got.dtype == np.float64 and got.shape == A.shape
    ratio = check("update_spatial (70, 129, 21)", "A", got.astype(F32), want, tol)
    assert np.array_equal(got.astype(F32).astype(np.float64), got)          # fp32 values in a float64 array
    assert not got[P // 2].any() and not got[3].any() and (tol[want != 0] > 0).all()
    print(f"\nupdate_spatial: |error| / bound {ratio:.3g}; host {t1 - t0:.3f} s, GPU {time.perf_counter() - t1:.3f} s")
