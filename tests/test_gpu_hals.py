"""K4h (exact NNLS trace solver, dnmf_hals_temporal*) on the GPU against its float64 restatement
(tests/hals_restatement.py) run on the very same G, r, C0.

Tolerances:
  fp32 C   |d| <= 1e-6 max|C| per frame  (one fp32 rounding, 6e-8, of an fp64 result, with an order of magnitude of room)
  fp64 C   |d| <= 1e-10 max|C| per frame (step form: fp64 sums in another order)
  kkt      |d| <= 1e-10 S_t, S_t = max(|r_t|, max_k sum_l |G_t[k,l]| c_l): the gradient is a sum of at most K + 3 <= 259
           terms no larger than S_t, each rounding 1.1e-16 of it, on states that themselves agree to ~1e-15
"""
import numpy as np
import pytest
import torch

import hals_restatement as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


@pytest.fixture(scope="module")
def ops(M):
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def close_per_frame(got, want, rel):
    """got, want (K,T): |d| <= rel * max|want| per frame; returns the worst ratio for the message."""
    d = np.abs(got - want).max(0)
    lim = rel * np.abs(want).max(0)
    print("max dev %.3e, limit at that frame %.3e" % (d.max(), lim[d.argmax()]))
    return bool((d <= lim).all())


def kkt_close(got, G, r, C, gamma=0.0):
    want = H.kkt(G, r, C, gamma)
    S = np.maximum(np.abs(r).max(1), np.einsum("tkl,lt->kt", np.abs(G), np.abs(C)).max(0))
    print("kkt dev %.3e of scale %.3e" % (np.abs(got - want).max(), S.max()))
    return bool((np.abs(got - want) <= 1e-10 * S).all())


_problems = {}


def problem(K, T):
    """(G (T,K,K), r (T,K), C0 (K,T)) fp32 numpy, made once per shape: G_t = a_t G0 + diag(b_t) with G0 = M^T M of a sparse
    non-negative M (symmetric, positive definite, different in every frame), r_t = G_t c* + noise.  From K = 5 on neuron 1
    has an all-zero row and column and r = 0 (d == 0: c must become 0) and neuron 3 has r so negative that its
    unconstrained optimum is negative whatever the others do (G, c >= 0): clamped to 0, with a positive gradient that kkt
    must not count."""
    if (K, T) not in _problems:
        rng = np.random.RandomState(1000 * K + T)
        Mx = rng.rand(2 * K + 20, K) * (rng.rand(2 * K + 20, K) < 0.3)
        G0 = Mx.T @ Mx
        G0 = (G0 + G0.T) / 2
        G = rng.uniform(0.5, 1.5, (T, 1, 1)) * G0[None] + np.eye(K)[None] * rng.uniform(0.2, 1.0, (T, K))[:, :, None]
        cs = rng.rand(K, T) * (rng.rand(K, T) > 0.3)
        r = np.einsum("tkl,lt->tk", G, cs) + 0.5 * rng.randn(T, K)
        if K >= 5:
            G[:, 1, :] = 0
            G[:, :, 1] = 0
            r[:, 1] = 0
            r[:, 3] = -5.0 - rng.rand(T)
        G32 = G.astype(np.float32)
        assert np.array_equal(G32, G32.transpose(0, 2, 1))
        _problems[(K, T)] = (G32, r.astype(np.float32), (0.05 + rng.rand(K, T)).astype(np.float32))
    return _problems[(K, T)]


@pytest.mark.parametrize("T", [1, 3, 70])
@pytest.mark.parametrize("K", [1, 5, 64, 65, 129, 256])
def test_dense_form(ops, K, T):
    """Every width the lanes split differently (K <= 64, one entry more, three per lane, the limit), one frame, fewer
    frames than a workgroup holds, and a partial last workgroup (70 = 17 x 4 + 2); iters 0, 1 and 7; C a view with
    ldc > T whose other columns stay as they are."""
    G, r, C0 = problem(K, T)
    Gd, rd = dev(G), dev(r)
    for iters in (0, 1, 7):
        buf = torch.full((K, T + 5), -7.0, device="cuda")
        C = buf[:, 2:2 + T]
        C.copy_(dev(C0))
        out, kkt = ops.hals_temporal(Gd, rd, C, iters, kkt=True)
        assert out is C
        assert bool((buf[:, :2] == -7).all()) and bool((buf[:, 2 + T:] == -7).all())
        want = H.hals_temporal(G, r, C0, 0.0, iters)
        if iters == 0:
            assert np.array_equal(host(C), C0.astype(np.float64))
        else:
            assert close_per_frame(host(C), want, 1e-6), (K, T, iters)
            assert bool((C >= 0).all())
        assert kkt.dtype == torch.float64 and tuple(kkt.shape) == (T,)
        assert kkt_close(host(kkt), G, r, want), (K, T, iters)
        if K >= 5 and iters > 0:
            assert bool((C[1] == 0).all()) and bool((C[3] == 0).all())
            g = H.gradient(G, r, want)                  # counting the clamped neuron's gradient would show
            assert (g[3] > 4.0).all() and (np.abs(g).max(0) - H.kkt(G, r, want) > 1e-3 * np.abs(r).max(1)).all()
        if iters == 7:   # without kkt, on a contiguous C: the same traces bit for bit
            assert torch.equal(ops.hals_temporal(Gd, rd, dev(C0), iters), C)


def test_clamped_neuron_stays_clamped(ops):
    G, r, C0 = problem(5, 3)
    a = ops.hals_temporal(dev(G), dev(r), dev(C0), 1)
    b = ops.hals_temporal(dev(G), dev(r), a.clone(), 30)
    assert bool((a[3] == 0).all()) and bool((b[3] == 0).all()) and bool((b[1] == 0).all())
    assert close_per_frame(host(b), H.hals_temporal(G, r, host(a), 0.0, 30), 1e-6)


def test_unsupported_K_names_the_call(ops):
    from dnmf_amd._lib import DnmfHipError
    K, T = 257, 2
    G, r = torch.zeros(T, K, K, device="cuda"), torch.zeros(T, K, device="cuda")
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_hals_temporal: K=257"):
        ops.hals_temporal(G, r, torch.zeros(K, T, device="cuda"), 1)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_hals_temporal_step: K=257"):
        ops.hals_temporal_step(G, r, torch.zeros(K, T, device="cuda", dtype=torch.float64), 0.1, 0)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_hals_temporal_kkt: K=257"):
        ops.hals_temporal_kkt(G, r, torch.zeros(K, T, device="cuda", dtype=torch.float64), 0.1)


# ---- compact footprints: the nbr and slot forms --------------------------------------------------------------------
# K Gaussian footprints in a chain along x, each cut to a box of `width` voxels starting at k * stride (all of y and z): two
# boxes meet (K3n's pattern: within one voxel of each other) while their indices differ by at most width // stride,
# which fixes the width of the pattern and with it NN: 5 -> 8, 11 -> 16, 21 -> 32.
CHAINS = {8: ([20, 16, 2], 9, 4, 2), 16: ([48, 16, 2], 20, 10, 2), 32: ([52, 12, 1], 40, 10, 1)}
_chains = {}


def chain(ops, NN, T=6):
    if NN not in _chains:
        sz, K, width, stride = CHAINS[NN]
        rng = np.random.RandomState(NN)
        X, Y, Z = sz
        x, y = np.arange(X)[:, None, None, None], np.arange(Y)[None, :, None, None]
        k = np.arange(K)[None, None, None, :]
        cx, cy = k * stride + (width - 1) / 2.0, rng.uniform(0.3, 0.7, K)[None, None, None, :] * Y
        A = np.exp(-((x - cx) ** 2) / (0.18 * width ** 2) - ((y - cy) ** 2) / (0.5 * Y ** 2)) * np.ones((1, 1, Z, 1))
        A = A * ((x >= k * stride) & (x < k * stride + width))
        assert (k * stride + width).max() <= X
        A = dev(A)
        ly = ops.pack_footprints_lists(A, sz)
        assert ly["nbr"] is not None and ly["nbr"].shape[1] == NN, ly["nbr"]
        beta = torch.cat((torch.zeros(1, 3), torch.eye(3), torch.zeros(6, 3)), 0)[:, :, None].repeat(1, 1, T)
        beta[0, :2, :] += torch.from_numpy(rng.uniform(-1.5, 1.5, (2, T))).float()     # a shift per frame in x and y
        beta = beta.cuda().contiguous()
        Ct = rng.rand(K, T) * (rng.rand(K, T) > 0.3)
        frames = (A.reshape(-1, K).double() @ dev(Ct, torch.float64)).T + 0.2 * dev(rng.randn(T, X * Y * Z), torch.float64)
        frames = frames.float().contiguous()
        G, r, _ = ops.warp_gram_rhs_lists(ly, K, sz, beta, None, frames)
        C0 = (0.05 + rng.rand(K, T)).astype(np.float32)
        _chains[NN] = dict(sz=sz, K=K, T=T, A=A, ly=ly, beta=beta, frames=frames, G=G.clone(), r=r.clone(), C0=C0)
    return _chains[NN]


@pytest.mark.parametrize("NN", [8, 16, 32])
def test_nbr_form_equals_dense_form(ops, NN):
    c = chain(ops, NN)
    G, r, C0, nbr = c["G"], c["r"], c["C0"], c["ly"]["nbr"]
    want = H.hals_temporal(host(G), host(r), C0, 0.0, 7)
    got, kkt = ops.hals_temporal(G, r, dev(C0), 7, nbr=nbr, kkt=True)
    dense, kkt_d = ops.hals_temporal(G, r, dev(C0), 7, kkt=True)
    assert close_per_frame(host(got), want, 1e-6) and close_per_frame(host(dense), want, 1e-6)
    assert close_per_frame(host(got), host(dense), 1e-6)
    assert kkt_close(host(kkt), host(G), host(r), want) and kkt_close(host(kkt_d), host(G), host(r), want)
    assert float(kkt.max()) < float(ops.hals_temporal(G, r, dev(C0), 0, nbr=nbr, kkt=True)[1].min())   # it descends
    # list entries outside [0,K) are skipped: put them where the padding (columns outside the pattern, exact zeros) was
    ly = c["ly"]
    pad = ~(ly["pair_slot"] != ly["nslot"] - 1).gather(1, nbr.long())
    assert bool(pad.any())
    bad = nbr.clone()
    bad[pad] = torch.where(torch.arange(int(pad.sum()), device="cuda") % 2 == 0, -1, c["K"] + 3).to(torch.int32)
    assert torch.equal(ops.hals_temporal(G, r, dev(C0), 7, nbr=bad), got)
    # the step form on the lists, with the neighbour term
    a = dev(C0, torch.float64)
    for _ in range(3):
        ops.hals_temporal_step(G, r, a, 0.7, 0, nbr=nbr)
        ops.hals_temporal_step(G, r, a, 0.7, 1, nbr=nbr)
    want = H.hals_temporal(host(G), host(r), C0, 0.7, 3)
    assert close_per_frame(host(a), want, 1e-10)
    assert kkt_close(host(ops.hals_temporal_kkt(G, r, a, 0.7, nbr=nbr)), host(G), host(r), want, 0.7)


@pytest.mark.parametrize("NN", [8, 16, 32])   # 20x16x2, 48x16x2 and 52x12x1 (Z = 1)
def test_slot_form_equals_dense_form(ops, NN):
    """K3n with finish=False, then K4h on its slot tables, against K3n with finish=True, then the dense form."""
    c = chain(ops, NN)
    ly, sz, K = c["ly"], c["sz"], c["K"]
    _, _, ws = ops.warp_gram_rhs_lists(ly, K, sz, c["beta"], None, c["frames"], finish=False)
    for iters in (0, 1, 7):
        got, kkt = ops.hals_temporal_slots(ly, ws, sz, dev(c["C0"]), iters, kkt=True)
        want = H.hals_temporal(host(c["G"]), host(c["r"]), c["C0"], 0.0, iters)
        assert close_per_frame(host(got), want, 1e-6), iters
        assert kkt_close(host(kkt), host(c["G"]), host(c["r"]), want), iters
        assert close_per_frame(host(got), host(ops.hals_temporal(c["G"], c["r"], dev(c["C0"]), iters)), 1e-6)
    assert torch.equal(ops.hals_temporal_slots(ly, ws, sz, dev(c["C0"]), 7), got)


# ---- the neighbour term: red-black half sweeps on an fp64 state ---------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 3, 6])
@pytest.mark.parametrize("K", [5, 65])
def test_step_form(ops, K, T):
    """Both parities, both ends and n_t = 0 (T = 1), 1 (ends), 2 (inside); parity 1 at T = 1 has no frame at all."""
    G, r, C0 = problem(K, T)
    gamma = 0.8
    Gd, rd = dev(G), dev(r)
    buf = torch.full((K, T + 3), -7.0, device="cuda", dtype=torch.float64)
    a = buf[:, 1:1 + T]
    a.copy_(dev(C0, torch.float64))
    for s in range(3):
        ops.hals_temporal_step(Gd, rd, a, gamma, 0)
        if s == 0:   # half a sweep: the odd frames are untouched
            assert np.array_equal(host(a)[:, 1::2], C0.astype(np.float64)[:, 1::2])
        ops.hals_temporal_step(Gd, rd, a, gamma, 1)
    assert bool((buf[:, :1] == -7).all()) and bool((buf[:, 1 + T:] == -7).all())
    want = H.hals_temporal(G, r, C0, gamma, 3)
    assert close_per_frame(host(a), want, 1e-10), (K, T)
    assert bool((a[3] == 0).all())       # (neuron 1, without a footprint, is the mean of its neighbours in time here)
    assert bool((a[1] == 0).all()) == (T == 1)
    assert kkt_close(host(ops.hals_temporal_kkt(Gd, rd, a, gamma)), G, r, want, gamma)
    assert kkt_close(host(ops.hals_temporal_kkt(Gd, rd, a, 0.0)), G, r, want, 0.0)
    if T > 1:
        assert not close_per_frame(want, H.hals_temporal(G, r, C0, 0.0, 3), 1e-6)   # the term is felt


# ---- through the public classes -------------------------------------------------------------------------------------

def model(M, c, cls=None, colours=None):
    sz, K, T = c["sz"], c["K"], c["T"]
    pos = torch.rand(K, 3) * torch.tensor(sz).float()
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos) if colours is None else \
        M.MultiChannelDNMF(torch.tensor(sz), K, T, colours, positions=pos)
    dn.verbose = False
    dn.fp.A = c["A"].clone()
    dn.fp.invalidate_layouts()
    with torch.no_grad():
        dn.fp.beta.copy_(c["beta"])
    dn.C = dev(c["C0"])
    return dn


def F(G, r, C):
    return H.objective(host(G), host(r), host(C))


def gram_tolerance(G, C):
    """Per frame, the bound on |C(K3n data) - C(K3 data)|: the fp32 tolerance of the traces, 1e-6 max|C|, plus the stated K3n-vs-K3
    difference of the Gram data, 2e-5 of the largest entry, times the condition number of G_t (what a relative change of the
    data of a linear system can do to its solution, to first order; about 7 on these footprints)."""
    cond = np.array([np.linalg.cond(g) for g in host(G)])
    return (1e-6 + 2e-5 * cond) * np.abs(host(C)).max(0)


def lists_gram(M, c, colours=None):
    """K3n's own finished G, r of the model of `c` (the data the slot path reads, entry for entry)."""
    ref = model(M, c, colours=colours)
    ref.gram_kernel = "lists"
    return ref._gram_rhs(c["frames"], torch.arange(c["T"], dtype=torch.int32, device="cuda"))


def test_update_footprints_hals(M, ops, capsys):
    """20x16x2, K = 9, T = 12 on simulated frames: the slot path (gram_kernel='lists') and the dense-G path ('dense') agree,
    end lower in F than the multiplicative update from the same start, and report last_temporal_kkt."""
    c = chain(ops, 8, T=6)
    c = dict(c)
    # T = 12: the six frames twice, the second half under other shifts
    c["T"] = 12
    c["beta"] = torch.cat((c["beta"], c["beta"].flip(2)), 2).contiguous()
    c["frames"] = torch.cat((c["frames"], c["frames"]), 0).contiguous()
    c["C0"] = np.concatenate((c["C0"], c["C0"][::-1]), 1).copy()
    sz, K, T = c["sz"], c["K"], c["T"]
    assert (sz, K, T) == ([20, 16, 2], 9, 12)
    loader = M.ResidentLoader(c["frames"], sz, 4)
    out = {}
    for kernel in ("lists", "dense"):
        for solver in ("hals", "mu"):
            dn = model(M, c)
            dn.gram_kernel = kernel
            assert (dn._lists_layout_for_fused_update(0) is not None) == (kernel == "lists")
            dn.update_footprints(loader, 4, sz, gamma_c=0, iter_c=10, return_dense=False, solver=solver)
            out[kernel, solver] = dn.C.clone()
            if solver == "hals":
                kkt = dn.last_temporal_kkt
                assert kkt is not None and tuple(kkt.shape) == (T,) and kkt.dtype == torch.float64 and not kkt.is_cuda
                assert bool(torch.isfinite(kkt).all()) and bool((kkt >= 0).all())
            else:
                assert dn.last_temporal_kkt is None
    ref = model(M, c)
    ref.gram_kernel = "dense"
    order = torch.arange(T, dtype=torch.int32, device="cuda")
    G, r = ref._gram_rhs(c["frames"], order)
    d = np.abs(host(out["lists", "hals"]) - host(out["dense", "hals"])).max(0)
    tol = gram_tolerance(G, out["dense", "hals"])
    print("lists vs dense: dev", d.max(), "tolerance", tol.min())
    assert (d <= tol).all()
    # the slot path against the restatement on K3n's own finished G, r: the slot tables hold those sums entry for entry
    Gn, rn = lists_gram(M, c)
    assert close_per_frame(host(out["lists", "hals"]), H.hals_temporal(host(Gn), host(rn), c["C0"], 0.0, 10), 1e-6)
    assert not close_per_frame(host(out["lists", "hals"]), H.hals_temporal(host(Gn), host(rn), c["C0"], 0.0, 9), 1e-6)
    assert close_per_frame(host(out["dense", "hals"]), H.hals_temporal(host(G), host(r), c["C0"], 0.0, 10), 1e-6)
    for kernel in ("lists", "dense"):
        f_h, f_m, f_0 = F(G, r, out[kernel, "hals"]), F(G, r, out[kernel, "mu"]), F(G, r, dev(c["C0"]))
        print(kernel, "F hals %.9g mu %.9g start %.9g" % (f_h, f_m, f_0))
        assert f_h <= f_m < f_0
    # verbose prints one line with the measure
    dn = model(M, c)
    dn.verbose = True
    capsys.readouterr()
    dn.update_footprints(loader, 4, sz, gamma_c=0, iter_c=2, return_dense=False, solver="hals")
    text = capsys.readouterr().out
    lines = [ln for ln in text.splitlines() if "KKT" in ln]
    assert len(lines) == 1 and "max" in lines[0] and "median" in lines[0]
    with pytest.raises(ValueError, match="solver="):
        dn.update_footprints(loader, 4, sz, gamma_c=0, iter_c=2, return_dense=False, solver="nnls")
    # with the neighbour term: red-black sweeps on an fp64 copy, rounded to fp32 at the end
    dn = model(M, c)
    dn.gram_kernel = "dense"
    dn.update_footprints(loader, 4, sz, gamma_c=0.5, iter_c=4, return_dense=False, solver="hals")
    want = H.hals_temporal(host(G), host(r), c["C0"], 0.5, 4)
    assert close_per_frame(host(dn.C), want, 1e-6)
    assert kkt_close(dn.last_temporal_kkt.numpy(), host(G), host(r), want, 0.5)
    # fit forwards the option
    dn = model(M, c)
    dn.update_motion = lambda *a, **k: None
    dn.fit([], loader, None, 4, outer=1, epochs=0, gamma_c=0, iter_c=10, solver="hals")
    assert dn.last_temporal_kkt is not None and torch.equal(dn.C, out["lists", "hals"])


def test_update_footprints_hals_two_colours(M, ops):
    c = dict(chain(ops, 8, T=6))
    sz, K, T = c["sz"], c["K"], c["T"]
    colours = torch.tensor(np.random.RandomState(5).uniform(0.3, 1.0, (2, K))).float()
    c["frames"] = torch.cat([c["frames"] * float(s) for s in (1.0, 0.6)], 1).contiguous()   # rows of 2 P floats
    loader = M.ResidentLoader(c["frames"], sz, 4)
    out = {}
    for kernel in ("lists", "dense"):
        for solver in ("hals", "mu"):
            dn = model(M, c, colours=colours)
            dn.gram_kernel = kernel
            dn.update_footprints(loader, 4, sz, gamma_c=0, iter_c=10, solver=solver)
            out[kernel, solver] = dn.C.clone()
            assert (dn.last_temporal_kkt is not None) == (solver == "hals")
    ref = model(M, c, colours=colours)
    ref.gram_kernel = "dense"
    G, r = ref._gram_rhs(c["frames"], torch.arange(T, dtype=torch.int32, device="cuda"))
    d = np.abs(host(out["lists", "hals"]) - host(out["dense", "hals"])).max(0)
    assert (d <= gram_tolerance(G, out["dense", "hals"])).all()
    Gn, rn = lists_gram(M, c, colours=colours)
    assert close_per_frame(host(out["lists", "hals"]), H.hals_temporal(host(Gn), host(rn), c["C0"], 0.0, 10), 1e-6)
    assert close_per_frame(host(out["dense", "hals"]), H.hals_temporal(host(G), host(r), c["C0"], 0.0, 10), 1e-6)
    for kernel in ("lists", "dense"):
        assert F(G, r, out[kernel, "hals"]) <= F(G, r, out[kernel, "mu"]) < F(G, r, dev(c["C0"]))


def test_solver_mu_is_the_path_as_it_was(M, ops):
    """solver='mu' and no solver argument: the traces of a direct K3n + K4 / K3 + K4 call, bit for bit."""
    c = chain(ops, 8, T=6)
    sz, K, T = c["sz"], c["K"], c["T"]
    loader = M.ResidentLoader(c["frames"], sz, 4)
    order = torch.arange(T, dtype=torch.int32, device="cuda")
    for kernel, gamma in (("lists", 0), ("dense", 0), ("dense", 0.01), ("lists", 0.01)):
        got = []
        for kw in ({}, {"solver": "mu"}):
            dn = model(M, c)
            dn.gram_kernel = kernel
            dn.update_footprints(loader, 4, sz, gamma_c=gamma, iter_c=5, return_dense=False, **kw)
            got.append(dn.C.clone())
            assert dn.last_temporal_kkt is None
        dn = model(M, c)
        dn.gram_kernel = kernel
        if kernel == "lists" and gamma == 0:
            ly = dn.fp.packed_lists()
            _, _, ws = ops.warp_gram_rhs_lists(ly, K, sz, dn.fp.beta.detach(), order, c["frames"], finish=False)
            want = ops.mu_temporal_slots(ly, ws, sz, dev(c["C0"]), 5)
        else:
            G, r = dn._gram_rhs(c["frames"], order)
            want = M._mu_temporal(G, r, dev(c["C0"]), gamma, 5, nbr=dn._gram_nbr)
        assert torch.equal(got[0], want) and torch.equal(got[1], want), (kernel, gamma)


def test_static_update_temporal_hals(M, ops):
    """numpy in, float64 numpy out, against the restatement on the very G, r the method forms (K3 without a warp on the same
    arrays, as update_temporal calls it): fp64 state throughout, so 1e-10; one sweep fewer is far outside that."""
    rng = np.random.RandomState(8)
    A_t, C, Y = rng.rand(6, 5, 2, 4, 3), 0.3 + rng.rand(4, 3), rng.rand(6, 5, 2, 3)
    A_dev = dev(np.moveaxis(A_t, 4, 0).reshape(3, 60, 4))
    Apk = ops.pack_footprints(A_dev)
    G, r = ops.warp_gram_rhs(Apk, 4, (6, 5, 2), None, [0, 1, 2], dev(np.moveaxis(Y, 3, 0).reshape(3, 60)),
                             a_frame_stride=60 * Apk.shape[1])[:2]
    G, r = host(G), host(r)
    for gamma in (None, 0.4):
        got = M.DeformableNMF.update_temporal(A_t, C, Y, gamma=gamma, solver='hals', iters=6)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (4, 3)
        assert close_per_frame(got, H.hals_temporal(G, r, C, gamma, 6), 1e-10)
        assert not close_per_frame(got, H.hals_temporal(G, r, C, gamma, 5), 1e-6)
    # iters rounds of the multiplicative update are iters calls of the method as it was
    two = M.DeformableNMF.update_temporal(A_t, M.DeformableNMF.update_temporal(A_t, C, Y), Y)
    np.testing.assert_allclose(M.DeformableNMF.update_temporal(A_t, C, Y, iters=2), two, rtol=1e-12)
