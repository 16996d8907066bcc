"""K21 on the GPU: ``ops.deconvolve_traces`` against the float64 restatement (tests/deconv_restatement.py) on identical seeded
inputs, and ``DeformableNMF.deconvolve``.

The input rows are a view into a wider buffer filled with 1e6, so that a read past a row shows.  Three modes per size: g, penalty and
baseline given; g given and the rest estimated; everything estimated.

With g, penalty and baseline given, c and s are within one fp32 ulp of the restatement's fp32 rounding plus 1e-9 max|y - b| (the
rounding of at most 2e4 float64 terms through a non-expansive projection stays below 1e-11: two decades are left), the RSS within
1e-10 relative.  With estimates: noise and baseline within 1e-12 relative (a selection and one or two roundings), g within 1e-10,
the penalty within 1e-8 max(noise, penalty) (32 halvings of a bracket of at most 2 penalty or noise give 5e-10), c and s within
1e-7 max|y - b|; ``ok`` and the NaN rows are equal.

Largest deviations measured on the MI355X: see README.md (K21); the tests print them.
"""
import functools

import numpy as np
import pytest
import torch

import deconv_restatement as DR

pytestmark = pytest.mark.gpu

G = float(np.exp(-0.3))
# 1023 .. 1025: one frame a lane, then the first size with two; 6144 / 6145: the last size with the records in LDS, the first with
# them in the workspace
SIZES = [1, 2, 63, 65, 257, 1000, 1023, 1024, 1025, 4099, 6144, 6145]
MODES = ["given", "g_given", "estimated"]
LAM = 0.3
BASE = np.array([1.0, 1.0, 1.0, 7.25, 0.0, 0.0, 0.0, 1.0])      # the baselines of the rows of make_traces, for the mode "given"


def spikes_trace(rng, T, noise):
    s = (rng.rand(T) < 0.1).astype(np.float64)
    c = np.zeros(T)
    for t in range(T):
        c[t] = (G * c[t - 1] if t else 0.0) + s[t]
    return 1.0 + c + noise * rng.randn(T)


def make_traces(T, seed):
    """Eight rows: 0 simulated spikes plus noise; 1 the same with a leading run, an interior gap that empties whole segments of
    lanes, the last frame and 10 % at random missing; 2 all NaN; 3 constant; 4 a decay faster than g (one pool across every
    boundary); 5 strictly increasing (every frame a pool of its own); 6 negative (c = 0 above the baseline 0); 7 simulated, more
    noise."""
    rng = np.random.RandomState(seed)
    t = np.arange(T)
    x = np.empty((8, T))
    x[0] = spikes_trace(rng, T, 0.1)
    x[1] = spikes_trace(rng, T, 0.1)
    x[1, :min(3, T)] = np.nan
    x[1, T // 3:T // 3 + max(T // 8, 2)] = np.nan                 # at T = 4099 (5 frames a lane) a hundred lanes without a sample
    x[1, T - 1] = np.nan
    x[1, rng.rand(T) < 0.1] = np.nan
    x[2] = np.nan
    x[3] = 7.25
    x[4] = 3.0 * (0.9 * G) ** t
    x[5] = 1.0 + 0.01 * t
    x[6] = -1.0 - np.abs(rng.randn(T))
    x[7] = spikes_trace(rng, T, 0.3)
    if T > 20:
        x[7, 10] = np.inf                                         # not finite: missing
        x[7, 11] = -np.inf
    return x.astype(np.float32)


def rows_of(T, mode):
    """The rows of a case: all eight, at the longest size half of them for the modes that search the penalty."""
    return [0, 1, 3, 4] if (T > 2000 and mode != "given") else list(range(8))


def options(mode, rows):
    if mode == "given":
        return dict(g=G, penalty=LAM, baseline=BASE[rows])
    return dict(g=G) if mode == "g_given" else {}


@functools.lru_cache(maxsize=None)
def reference(T, mode):
    """The restatement on a case -> (input, its result); computed once, never changed."""
    rows = rows_of(T, mode)
    x = make_traces(T, 1000 + T)[rows]
    return x, DR.deconvolve_traces(x, **options(mode, rows))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def strided(x, pad=5):
    buf = torch.full((x.shape[0], x.shape[1] + pad), 1.0e6, dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf, buf[:, :x.shape[1]]


def to_gpu_options(opt):
    return {k: (torch.from_numpy(np.asarray(v, np.float64)).cuda() if isinstance(v, np.ndarray) else v) for k, v in opt.items()}


def scale_of(x, b):
    """max |y - b| per row over the valid frames (1 for a row without one)."""
    w = np.isfinite(x)
    d = np.where(w, np.abs(np.where(w, x, 0.0).astype(np.float64) - np.where(np.isnan(b), 0.0, b)[:, None]), 0.0)
    return np.where(w.any(axis=1), d.max(axis=1), 1.0)


def compare(x, got, want, mode):
    """Assert the bounds of the module docstring -> the largest deviation of each kind."""
    c, s, info = got
    wc, ws, w = want
    c, s = c.cpu().numpy(), s.cpu().numpy()
    gi = {k: v.cpu().numpy() for k, v in info.items() if k != "workspace"}
    assert c.dtype == s.dtype == np.float32 and c.shape == s.shape == x.shape
    assert gi["g"].dtype == gi["rss"].dtype == np.float64 and gi["n_valid"].dtype == gi["n_pools"].dtype == np.int32 and gi["ok"].dtype == bool
    ok = w["ok"].astype(bool)
    np.testing.assert_array_equal(gi["ok"], ok)
    np.testing.assert_array_equal(gi["n_valid"], w["n_valid"])
    np.testing.assert_array_equal(np.isnan(c), np.isnan(wc))
    np.testing.assert_array_equal(np.isnan(s), np.isnan(ws))
    assert np.isnan(c[~ok]).all() and not np.isnan(c[ok]).any()
    for key in ("g", "penalty", "baseline", "noise", "rss"):
        np.testing.assert_array_equal(np.isnan(gi[key]), np.isnan(w[key]), err_msg=key)
    dev = dict(c=0.0, s=0.0, rss=0.0, noise=0.0, baseline=0.0, g=0.0, penalty=0.0)
    if not ok.any():
        return dev
    scale = scale_of(x, w["baseline"])

    def rel(a, b):
        m = ok & ~np.isnan(b) & (a != b)
        return float((np.abs(a - b)[m] / np.abs(b)[m]).max()) if m.any() else 0.0

    if mode == "given":
        for name, a, b in (("c", c, wc), ("s", s, ws)):
            b32 = b[ok].astype(np.float32)
            allow = np.spacing(np.abs(b32)).astype(np.float64) + 1e-9 * scale[ok][:, None]
            err = np.abs(a[ok].astype(np.float64) - b32.astype(np.float64))
            dev[name] = float((err / allow).max())
            assert dev[name] <= 1.0, (name, dev[name])
        dev["rss"] = rel(gi["rss"], w["rss"])
        assert dev["rss"] <= 1e-10
        np.testing.assert_array_equal(gi["g"][ok], w["g"][ok])
        np.testing.assert_array_equal(gi["penalty"][ok], w["penalty"][ok])
        np.testing.assert_array_equal(gi["baseline"][ok], w["baseline"][ok])
        np.testing.assert_array_equal(gi["n_pools"][ok], w["n_pools"][ok])
    else:
        dev["noise"], dev["baseline"] = rel(gi["noise"], w["noise"]), rel(gi["baseline"], w["baseline"])
        assert dev["noise"] <= 1e-12 and dev["baseline"] <= 1e-12, dev
        dev["g"] = float(np.abs(gi["g"] - w["g"])[ok].max())
        assert dev["g"] <= 1e-10
        lam_allow = 1e-8 * np.maximum(w["noise"], w["penalty"])[ok]
        lam_err = np.abs(gi["penalty"] - w["penalty"])[ok]
        dev["penalty"] = float(np.where(lam_err > 0, lam_err / np.where(lam_allow > 0, lam_allow, 1e-300), 0.0).max())
        assert dev["penalty"] <= 1.0, (gi["penalty"], w["penalty"])
        for name, a, b in (("c", c, wc), ("s", s, ws)):
            err, allow = np.abs(a[ok].astype(np.float64) - b[ok]), np.broadcast_to(1e-7 * scale[ok][:, None], b[ok].shape)
            dev[name] = float(np.where(err > 0, err / np.where(allow > 0, allow, 1e-300), 0.0).max())      # a constant row allows nothing
            assert dev[name] <= 1.0, (name, dev[name])
    return dev


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", SIZES)
def test_deconvolve_against_the_restatement(ops, T, mode):
    rows = rows_of(T, mode)
    x, want = reference(T, mode)
    opt = to_gpu_options(options(mode, rows))
    buf, view = strided(x)
    before = buf.clone()
    got = ops.deconvolve_traces(view, **opt)
    again = ops.deconvolve_traces(view.contiguous(), **opt)
    torch.cuda.synchronize()
    # the input is unchanged; a second call (on a contiguous copy) returns the same bits
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    assert torch.equal(got[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))
    for key in ("g", "penalty", "baseline", "noise", "rss"):
        assert torch.equal(got[2][key].view(torch.int64), again[2][key].view(torch.int64)), key
    assert torch.equal(got[2]["n_pools"], again[2]["n_pools"])
    dev = compare(x, got, want, mode)
    print(f"T={T} {mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()) + "  (c, s, penalty: share of the allowance)")
    if T < 4:
        assert not want[2]["ok"].any()                            # fewer than 4 frames: every row refused
    elif mode != "estimated":
        assert want[2]["ok"].sum() == len(rows) - (2 in rows)     # every row but the all-NaN one


def test_the_special_rows_are_what_they_are_meant_to_be():
    """On the restatement (the cases are this file's): one pool across every boundary, a pool per frame, c = 0, no penalty on the
    constant row, the refusals of the mode that estimates g."""
    x, (c, s, w) = reference(4099, "given")
    assert not w["ok"][2] and w["n_valid"][2] == 0
    assert w["n_pools"][4] == 1 and w["n_pools"][5] >= 4098 and (c[6] == 0).all() and (c[3] == 0).all()
    gap = np.flatnonzero(np.isnan(x[1]))
    assert np.isnan(x[1, 4099 // 3:4099 // 3 + 512]).all() and len(gap) > 800      # a hundred lanes of 5 frames without a sample
    assert (s[1][gap] == 0).all() and (c[1][gap[gap > 3]] > 0).any()
    x, (c, s, w) = reference(1000, "g_given")
    assert w["ok"][3] and w["noise"][3] == 0 and w["penalty"][3] == 0 and w["baseline"][3] == 7.25
    assert (w["penalty"][[0, 1, 7]] > 0).all()                    # the search ran
    x, (c, s, w) = reference(1000, "estimated")
    assert not w["ok"][2] and not w["ok"][3] and w["ok"][[0, 1, 7]].all()
    assert (np.abs(w["g"][[0, 1]] - G) < 0.15).all()


def test_workspace_form_and_the_size_limit(ops):
    """T = 18 432: the pool records live in the workspace (18 frames a lane); one frame more is refused."""
    T = 18432
    rng = np.random.RandomState(77)
    x = np.stack([spikes_trace(rng, T, 0.1), spikes_trace(rng, T, 0.2)]).astype(np.float32)
    x[1, :5] = np.nan
    x[1, 6000:6700] = np.nan
    x[1, -1] = np.nan
    x[1, rng.rand(T) < 0.1] = np.nan
    want = DR.deconvolve_traces(x, g=G, penalty=LAM, baseline=1.0)
    buf, view = strided(x)
    got = ops.deconvolve_traces(view, g=G, penalty=LAM, baseline=1.0)
    again = ops.deconvolve_traces(view, g=G, penalty=LAM, baseline=1.0, workspace=got[2]["workspace"])
    torch.cuda.synchronize()
    assert got[2]["workspace"].numel() * 8 >= 2 * T * 24 and again[2]["workspace"] is got[2]["workspace"]
    assert torch.equal(got[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))
    dev = compare(x, got, want, "given")
    print(f"T={T} given, workspace form: " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    from dnmf_amd._lib import DnmfHipError
    with pytest.raises(DnmfHipError, match="dnmf_deconvolve_traces_workspace"):
        ops.deconvolve_traces(torch.zeros((1, T + 1), dtype=torch.float32, device="cuda"), g=G, penalty=LAM)


def test_model_deconvolve(ops):
    """``DeformableNMF.deconvolve`` on a small fitted model returns what ``ops.deconvolve_traces(model.C, ...)`` returns, stores
    ``last_deconv`` and leaves ``model.C`` bit-identical; on the output of ``clean_traces`` it works through the NaNs."""
    from dnmf_amd.Demix import dNMF as M
    sz, K, T = (24, 20, 2), 6, 40
    pos = torch.tensor([[5.0, 5.0, 0.0], [12.0, 6.0, 1.0], [19.0, 5.0, 0.0], [6.0, 14.0, 1.0], [12.0, 14.0, 0.0], [18.0, 15.0, 1.0]])
    rng = np.random.RandomState(7)
    truth = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    truth.C = torch.from_numpy(np.stack([0.2 + spikes_trace(rng, T, 0.02) for _ in range(K)])).to("cuda", torch.float32)
    with torch.no_grad():
        video = truth.fp.forward(range(T), truth.C)[0].reshape(T, -1).clone()
    model = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    model.verbose = False
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), iter_c=20)
    C = model.C.clone()
    assert model.last_deconv is None
    fps, decay_time = 4.0, 1.0 / (4.0 * 0.3)
    c, s, info = model.deconvolve(fps=fps, decay_time=decay_time, penalty=0.01)
    assert torch.equal(model.C.view(torch.int32), C.view(torch.int32))
    want = ops.deconvolve_traces(C, g=float(np.exp(-1.0 / (decay_time * fps))), penalty=0.01)
    assert torch.equal(c.view(torch.int32), want[0].view(torch.int32)) and torch.equal(s.view(torch.int32), want[1].view(torch.int32))
    assert model.last_deconv is info and sorted(info) == ["baseline", "g", "n_pools", "n_valid", "noise", "ok", "penalty", "rss"]
    assert torch.equal(info["rss"].view(torch.int64), want[2]["rss"].view(torch.int64)) and bool(info["ok"].all())
    assert abs(float(info["g"][0]) - G) < 1e-15 and bool((s >= 0).all()) and bool((s > 0).any())
    # after the clean-up: the trimmed frames are NaN, a leading run; the trace starts with the first valid frame
    cleaned = model.clean_traces(fps, detrend_mode=0)[0]
    lead = int(torch.isnan(cleaned[0]).float().argmin())
    assert lead >= 2 and bool(torch.isnan(cleaned[:, -1]).all())
    c2, s2, info2 = model.deconvolve(traces=cleaned, g=G)
    assert bool(info2["ok"].all()) and not bool(torch.isnan(c2).any()) and bool((c2[:, :lead] == 0).all()) and bool((s2[:, -1] == 0).all())
    assert int(info2["n_valid"][0]) == int((~torch.isnan(cleaned[0])).sum()) and model.last_deconv is info2
    assert torch.equal(model.C.view(torch.int32), C.view(torch.int32))
    # the reference-style entry point: numpy in, numpy out
    from Demix.Traces import deconvolveTraces
    c3, s3, info3 = deconvolveTraces(cleaned.cpu().numpy(), g=G)
    assert isinstance(c3, np.ndarray) and c3.dtype == np.float32 and np.array_equal(c3.view(np.int32), c2.cpu().numpy().view(np.int32))
    assert isinstance(info3["ok"], np.ndarray) and info3["ok"].all()
