"""K20 on the GPU: ``ops.clean_traces`` against the float64 restatement (tests/traces_restatement.py) on identical seeded inputs,
and ``DeformableNMF.clean_traces``.

The input rows are a view into a wider buffer filled with NaN, so that a read past a row shows.  Masks, ``n_outliers``, ``fitted``
and the sign of ``b`` must be equal; the inputs sit on no threshold (asserted on the restatement: every ``|d_t|`` is at least
``1e-6 thr`` away from ``thr``, no count of valid running-median entries equals ``0.1 T``).  ``F0`` (a percentile: one selection,
one interpolation) agrees within two float64 roundings.  ``a``, ``b``, ``scales`` and ``offsets`` come from the same float64
iteration and differ by the order of the sums and the last bit of ``exp`` / ``log``.

Worst relative deviation measured on these inputs on the MI355X: 1.8e-14 (b of the case K = 3, T = 7, where four samples carry
the fit; scales 1.4e-14 there; every other case stays below 2e-15: a 5.6e-16, b 1.9e-15, scales 1.8e-15, offsets 2.2e-16).  Ten
times the worst is allowed (MEASURED below), and at most 1e-9.  The sign of ``b`` is a branch like the two thresholds: the
restatement's ``b`` is asserted to be exactly 0 (a constant running median) or at least 1e-6 / T in magnitude.
The output traces are within one fp32 ulp of the restatement's value plus that allowance carried through the subtraction of the
curve (|a| (1 + |b| T) of it) and the division by the range.
"""
import functools

import numpy as np
import pytest
import torch

import traces_restatement as TR

pytestmark = pytest.mark.gpu

MEASURED = 1.8e-14      # worst relative deviation of a, b, scales, offsets over CASES, as printed by the tests on the MI355X
TOL = min(10 * MEASURED, 1e-9)
EPS = np.finfo(np.float64).eps

# (K, T, fps, options)
CASES = [
    (3, 1, 1.0, dict()),
    (1, 2, 0.7, dict()),
    (3, 2, 4.0, dict(detrend_mode=0)),
    (3, 3, 0.7, dict(detrend_mode=0)),
    (1, 3, 0.7, dict(detrend_mode=2, trim=False)),
    (3, 7, 0.7, dict()),                                                        # W = 7 = T
    (1, 7, 4.0, dict(detrend_mode=3)),                                          # W = 40 > T
    (65, 7, 1.0, dict(detrend_mode=1)),
    (65, 64, 1.0, dict(sigma_threshold=3.0)),                                   # W = 10, even
    (3, 64, 0.7, dict(detrend_mode=1)),
    (1, 64, 4.0, dict(sigma_threshold=None, contiguous=True)),
    (3, 64, 30.0, dict(detrend_mode=3, interp_method="linear")),                # W = 300 > T, every frame but the last trimmed
    (65, 257, 4.0, dict(detrend_mode=3, interp_method="linear")),
    (3, 257, 1.0, dict(sigma_threshold=3.0, smooth_method="movmean", smooth_window=5)),
    (3, 257, 0.7, dict(interp_method="linear", smooth_method="movmedian", smooth_window=4)),
    (65, 1000, 4.0, dict()),
    (3, 1000, 4.0, dict(detrend_mode=1, interp_method="linear", smooth_method="movmedian", smooth_window=5)),
    (1, 1000, 30.0, dict(detrend_mode=3, smooth_method="movmean", smooth_window=4)),   # W = 300
    (3, 1000, 0.7, dict(detrend_mode=0, interp_method="linear", smooth_method="movmedian", smooth_window=3)),
    (3, 2500, 4.0, dict(sigma_threshold=5.0, interp_method="linear", smooth_method="movmean", smooth_window=7)),   # a lane owns several frames
]


def make_traces(K, T, seed):
    """Decaying traces with transients, noise, single-frame jumps, dropouts and entries that are not finite; from K = 3 on (and
    T >= 64) special rows: a constant one and a rising one, from K = 65 on also an all-NaN one, one with five valid samples (no
    fit where 0.1 T exceeds the window) and one quantised to a few levels (equal values around every median)."""
    rng = np.random.RandomState(seed)
    t = np.arange(T)
    tau = rng.uniform(0.3, 3.0, K) * max(T, 8)
    x = (20.0 + 3.0 * rng.rand(K, T)) * np.exp(-t[None, :] / tau[:, None]) * rng.uniform(0.5, 4.0, K)[:, None]
    for k in range(K):
        for s in rng.choice(T, max(T // 40, 1), replace=False):
            x[k, s:s + 6] += rng.uniform(5.0, 20.0) * np.exp(-np.arange(len(x[k, s:s + 6])) / 2.0)
    if T >= 64:
        for k in range(0, K, 2):                     # a jump of a single frame, both ways
            s = rng.randint(8, T - 8)
            x[k, s] += (1 if k % 4 else -0.9) * (x[k].mean() + 25.0 * x[k].std())
    x[rng.rand(K, T) < 0.03] = 0.0
    x[rng.rand(K, T) < 0.01] = np.nan
    if T > 20:
        x[0, 10] = np.inf
        x[0, 11] = -5.0
    if K >= 3 and T >= 64:
        x[1] = 7.25
        x[2] = (2.0 + 0.5 * rng.rand(T)) * np.exp(t / (2.0 * T))
    if K >= 65 and T >= 64:
        x[60] = np.nan
        x[61] = 0.0
        x[61, T // 2:T // 2 + 5] = [3.0, 4.0, 5.0, 6.0, 7.0]     # the median of three leaves three of them, rising
        x[62] = 8.0 * np.round(x[62] / 8.0)
        x[63] = 0.005                                # everything at or below the floor
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(i):
    """The restatement on case i -> (input, its result, the two threshold diagnostics); computed once, never changed."""
    K, T, fps, opt = CASES[i]
    opt = {k: v for k, v in opt.items() if k != "contiguous"}
    x = make_traces(K, T, 100 + i)
    res = TR.clean_traces(x, fps, **opt)
    return x, res, TR.LAST["tie"], list(TR.LAST["valid"])


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def rel(got, want):
    """Worst relative deviation over the entries where ``want`` is a number (0 where both are 0); the NaNs must coincide."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want) & (want != got)
    return float((np.abs(got - want)[ok] / np.abs(want)[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_clean_traces_against_the_restatement(ops, i):
    K, T, fps, opt = CASES[i]
    contiguous = opt.get("contiguous", False)
    opt = {k: v for k, v in opt.items() if k != "contiguous"}
    x, (want, w_scales, w_offsets, w), tie, valid = reference(i)
    mode = opt.get("detrend_mode", 2)
    # the inputs sit on no threshold
    assert tie >= 1e-6, tie
    assert all(n != 0.1 * T for n in valid), (valid, T)
    fb = w["b"][w["fitted"]]
    assert ((fb == 0) | (np.abs(fb) * T >= 1e-6)).all(), fb

    buf = torch.full((K, T + 5), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :T] = torch.from_numpy(x).cuda()
    rows = buf[:, :T].contiguous() if contiguous else buf[:, :T]
    before = buf.clone()
    out, scales, offsets, info = ops.clean_traces(rows, fps, **opt)
    again = ops.clean_traces(rows, fps, **opt)
    torch.cuda.synchronize()
    assert out.shape == (K, T) and out.dtype == torch.float32 and scales.dtype == offsets.dtype == torch.float64
    # the input is unchanged, a second call returns the same bits
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    assert torch.equal(out.view(torch.int32), again[0].view(torch.int32))
    for u, v in ((scales, again[1]), (offsets, again[2]), (info["a"], again[3]["a"]), (info["b"], again[3]["b"]),
                 (info["F0"], again[3]["F0"])):
        assert torch.equal(u.view(torch.int64), v.view(torch.int64))

    got = out.cpu().numpy().astype(np.float64)
    a, b, F0 = (info[k].cpu().numpy() for k in ("a", "b", "F0"))
    scales, offsets = scales.cpu().numpy(), offsets.cpu().numpy()
    # equal: masks, counts, flags, the branch b < 0
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(info["n_outliers"].cpu().numpy(), w["n_outliers"])
    np.testing.assert_array_equal(info["fitted"].cpu().numpy(), w["fitted"])
    np.testing.assert_array_equal(b < 0, w["b"] < 0)
    # the percentile: two float64 roundings
    assert np.array_equal(np.isnan(F0), np.isnan(w["F0"]))
    ok = ~np.isnan(F0)
    assert (np.abs(F0 - w["F0"])[ok] <= 2 * EPS * np.abs(w["F0"])[ok]).all()
    # the fit and what follows from it
    devs = dict(a=rel(a, w["a"]), b=rel(b, w["b"]), scales=rel(scales, w_scales), offsets=rel(offsets, w_offsets))
    print(f"case {i} K={K} T={T} fps={fps} {opt}: relative deviation " + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    assert max(devs.values()) <= TOL, devs
    # the traces: one fp32 ulp of the restatement's value, plus the allowance carried through the curve and the range
    subtracted = w["fitted"] & (w["b"] < 0)
    curve = np.where(subtracted, np.abs(w["a"]) * (1 + np.abs(w["b"]) * T), 0.0)
    if mode == 3:
        spread = w_scales
    elif mode == 1:                                  # a is in units of the first scaling: the range of the trace after S2
        first = TR.clean_traces(x, fps, **{**opt, "detrend_mode": 0, "interp_method": None, "smooth_method": None})[1]
        spread = w_scales / first
    else:
        spread = w_scales
    with np.errstate(all="ignore"):
        allow = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + TOL * (2 * (curve / spread)[:, None] + 4.0 + np.abs(want))
    ok = ~np.isnan(want)
    worst = float((np.abs(got - want)[ok] / allow[ok]).max()) if ok.any() else 0.0
    print(f"case {i}: traces at most {worst:.3f} of the allowance, {int(ok.sum())} of {K * T} entries valid")
    assert worst <= 1.0
    if mode < 3 and ok.any():
        assert got[ok].min() >= 0.05 - 1e-6 and got[ok].max() <= 0.95 + 1e-6


def test_the_special_rows_are_what_they_are_meant_to_be():
    """On the restatement (no GPU needed for the statement, but the cases are this file's): the constant row comes out NaN, the
    rising one is fitted with b > 0 and nothing subtracted, the five-sample row is not fitted where 0.1 T exceeds the window."""
    i = [c[:3] for c in CASES].index((65, 1000, 4.0))
    x, (want, scales, offsets, w), _, _ = reference(i)
    assert np.isnan(want[1]).all() and w["fitted"][1] and w["b"][1] == 0.0           # constant: 0 / 0, never a decay of rounding size
    assert w["fitted"][2] and w["b"][2] > 0 and not np.isnan(want[2, 5:-2]).any()
    assert np.isnan(want[60]).all() and not w["fitted"][60] and np.isnan(w["F0"][60])
    assert not w["fitted"][61] and w["n_outliers"][61] == 0
    assert np.isnan(want[63]).all()
    assert w["fitted"][62] and len(np.unique(x[62][x[62] > 0.01])) < 40               # equal values around the medians
    assert w["n_outliers"].sum() >= 10                                                # the planted jumps are met
    j = [c[:3] for c in CASES].index((65, 64, 1.0))
    assert reference(j)[1][3]["fitted"][61]                                           # there the window covers more than 0.1 T


def test_model_clean_traces(ops):
    """``DeformableNMF.clean_traces`` on a small fitted model returns what ``ops.clean_traces(model.C, ...)`` returns, stores
    ``last_clean`` and leaves ``model.C`` bit-identical."""
    from dnmf_amd.Demix import dNMF as M
    sz, K, T = (24, 20, 2), 6, 40
    pos = torch.tensor([[5.0, 5.0, 0.0], [12.0, 6.0, 1.0], [19.0, 5.0, 0.0], [6.0, 14.0, 1.0], [12.0, 14.0, 0.0], [18.0, 15.0, 1.0]])
    rng = np.random.RandomState(7)
    truth = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    truth.C = torch.from_numpy((0.6 + 0.3 * rng.rand(K, T)) * np.exp(-np.arange(T) / 60.0)[None, :]).to("cuda", torch.float32)
    with torch.no_grad():
        video = truth.fp.forward(range(T), truth.C)[0].reshape(T, -1).clone()
    model = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    model.verbose = False
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), iter_c=20)
    C = model.C.clone()
    assert model.last_clean is None
    out, scales, offsets = model.clean_traces(4.0, detrend_mode=2, interp_method="linear")
    assert torch.equal(model.C.view(torch.int32), C.view(torch.int32))
    want = ops.clean_traces(C, 4.0, detrend_mode=2, interp_method="linear")
    assert torch.equal(out.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(scales.view(torch.int64), want[1].view(torch.int64))
    assert torch.equal(offsets.view(torch.int64), want[2].view(torch.int64))
    assert sorted(model.last_clean) == ["F0", "a", "b", "fitted", "n_outliers"]
    assert torch.equal(model.last_clean["b"].view(torch.int64), want[3]["b"].view(torch.int64))
    valid = ~torch.isnan(out)
    assert bool(valid[:, 3:-2].all()) and not bool(valid[:, :3].any())          # two frames trimmed, the median of three takes a third
    assert float(out[valid].min()) >= 0.05 - 1e-6 and float(out[valid].max()) <= 0.95 + 1e-6
    # the reference's entry point: numpy in, numpy out; [] for "none"
    from Demix.Traces import cleanTraces
    tr, sc, of = cleanTraces(C.cpu().numpy(), 4.0, interp_method="linear", smooth_method=[], smooth_window=[])
    assert isinstance(tr, np.ndarray) and tr.dtype == np.float32 and np.array_equal(tr.view(np.int32), out.cpu().numpy().view(np.int32))
    tr2 = cleanTraces(C, 4.0, interp_method="linear")[0]
    assert tr2.is_cuda and torch.equal(tr2.view(torch.int32), out.view(torch.int32))
