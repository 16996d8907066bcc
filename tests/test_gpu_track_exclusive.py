"""K15x on the GPU against its float64 restatement (tests/track_exclusive_restatement.py), against K15 where there is nothing to
exclude, and the public entry points built on it."""
import ctypes

import numpy as np
import pytest
import torch

import track_exclusive_restatement as TX
import track_restatement as TR

pytestmark = pytest.mark.gpu

CASES = TX.gpu_cases()
ROUNDS = (1, 2)


@pytest.fixture(scope="module")
def refs():
    """The definition on every case, for one and for two rounds (the searches of round 1 are the last ones of a one-round call):
    computed once, never changed."""
    return {(name, R): TX.reference(case, R) for name, case in CASES.items() for R in ROUNDS}


def rows_of(frames, pad=3):
    """(T, X, Y, Z) -> padded CUDA rows: a (T, P) view of (T, P + pad) floats (ld > X Y Z), the padding poisoned."""
    T = frames.shape[0]
    P = int(np.prod(frames.shape[1:]))
    buf = torch.full((T, P + pad), float("nan"), device="cuda")
    buf[:, :P] = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32).reshape(T, P)).cuda()
    return buf[:, :P]


def gpu_exclusive(case, order, rounds, **kw):
    from dnmf_amd import ops
    frames = case["frames"]
    bg = case.get("background")
    out = ops.track_neurons_exclusive(rows_of(frames), frames.shape[1:], torch.from_numpy(np.ascontiguousarray(case["predict"])).cuda(),
                                      torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).cuda(), shape_std=case["sigma"],
                                      search=case["search"], rounds=rounds, times=case.get("times"),
                                      background=None if bg is None else torch.from_numpy(bg), **kw)
    pos, amp, peak, nsub = out
    assert pos.dtype == torch.float64 and amp.dtype == torch.float32 and peak.dtype == torch.float32 and nsub.dtype == torch.int32
    return pos.cpu().numpy(), amp.cpu().numpy(), peak.cpu().numpy(), nsub.cpu().numpy()


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_equals_restatement(refs, name, rounds):
    """With the restatement's own order: the same p* in every search, centres within 1e-3 voxel and amplitudes and peaks at rtol
    1e-3 (K15's bounds) plus rounds x SENS, the same neighbour counts.  The times case reads a strict subset of padded rows,
    every case rows with ld = X Y Z + 3.
    Measured on the MI355X, the worst over the cases: 1.4e-5 voxel (moving2), amplitude 3.1e-6 (moving2), peak 1.3e-6 (crowd, one
    round); the pairs 3.5e-6 voxel, 9.9e-7 and 7.4e-7."""
    ref = refs[name, rounds]
    # conditions on the input, met by the restatement alone: everything found, no pick decided by rounding
    assert np.isfinite(ref["positions"]).all() and ref["margin"].min() >= 1e-3
    pos, amp, peak, nsub = gpu_exclusive(CASES[name], ref["order"], rounds)
    assert np.isfinite(pos).all() and np.isfinite(amp).all() and np.isfinite(peak).all()
    dp = np.abs(pos - ref["positions"]).max()
    da = np.abs(amp / ref["amplitudes"] - 1).max()
    ds = np.abs(peak / ref["peaks"] - 1).max()
    print(f"{name}, {rounds} rounds: K = {pos.shape[0]}, max |p^ - p^_ref| {dp:.2e} voxel, amplitude deviation {da:.2e}, peak deviation "
          f"{ds:.2e}, up to {nsub.max()} neighbours in a region")
    # |delta| <= 1/2: the integer voxel is the rounded centre unless delta is within 1e-3 of a half; compare it where it is not
    clear = np.abs(ref["positions"] - ref["pstar"]) < 0.499
    np.testing.assert_array_equal(np.rint(pos)[clear], ref["pstar"][clear])
    np.testing.assert_array_equal(nsub, ref["n_subtracted"])
    assert dp <= 1e-3 + rounds * TX.SENS["positions"]
    assert da <= 1e-3 + rounds * TX.SENS["amplitudes"]
    assert ds <= 1e-3 + rounds * TX.SENS["peaks"]


def test_the_cases_cover_what_they_are_for(refs):
    assert refs["crowd", 2]["positions"].shape[0] == 70 and refs["crowd", 2]["n_subtracted"].max() > 16     # more than one chunk of tables
    assert CASES["moving3"]["frames"].shape[1] == 9                                   # an axis shorter than the filter window
    assert CASES["times"]["times"] == [2, 0] and CASES["times"]["frames"].shape[0] == 3
    assert (refs["border", 2]["pstar"][:, 1] < 6).all() and (refs["border", 2]["n_subtracted"] == 1).all()    # r = 6: boxes cut at y = 0


def k15(case, predict):
    from dnmf_amd import ops
    frames = case["frames"]
    pos, amp, peak = ops.track_neurons(rows_of(frames), frames.shape[1:], torch.from_numpy(np.ascontiguousarray(predict)).cuda(),
                                       shape_std=case["sigma"], search=case["search"])
    return pos.cpu().numpy(), amp.cpu().numpy(), peak.cpu().numpy()


def test_bit_for_bit_k15_where_nothing_is_subtracted(refs):
    """K = 1, and neurons farther apart than any region reaches: positions, amplitudes and peaks equal K15's bits."""
    case = dict(CASES["moving0"])
    case["predict"] = case["predict"][1:2]
    T = case["frames"].shape[0]
    got = gpu_exclusive(case, np.zeros((1, T), dtype=np.int32), 3)
    for a, b in zip(got[:3], k15(case, case["predict"])):
        np.testing.assert_array_equal(a, b)
    assert (got[3] == 0).all()
    case = CASES["moving3"]
    assert (refs["moving3", 2]["n_subtracted"] == 0).all()
    got = gpu_exclusive(case, refs["moving3", 2]["order"], 2)
    for a, b in zip(got[:3], k15(case, case["predict"])):
        np.testing.assert_array_equal(a, b)


def test_two_runs_give_the_same_bits(refs):
    a = gpu_exclusive(CASES["crowd"], refs["crowd", 2]["order"], 2)
    b = gpu_exclusive(CASES["crowd"], refs["crowd", 2]["order"], 2)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("pair", range(len(TX.PAIRS)))
def test_track_positions_with_exclude_finds_both_neurons_of_a_pair(pair):
    """The class level reproduces the thresholds of tests/test_track_exclusive_host.py; its order, from the GPU's K15 peaks, is the
    reference's: per frame the two K15 peaks differ by more than 1e-2 relative, or K15 picked the same voxel for both and they
    are the same number."""
    from dnmf_amd.Demix.dNMF import ExponentialFP
    frames, rest, truth, amps, sigma, search = TX.pair_case(pair)
    ref15 = TR.track(frames, rest, sigma, search)
    gap = np.abs(ref15["peaks"][0] / ref15["peaks"][1] - 1)
    same = (ref15["pstar"][0] == ref15["pstar"][1]).all(0)
    assert ((gap > 1e-2) | same).all()
    case = dict(frames=frames, sigma=sigma, search=search)
    order = torch.argsort(torch.from_numpy(k15(case, rest)[2]), dim=0, descending=True, stable=True).numpy()
    np.testing.assert_array_equal(order, TX.default_order(ref15["peaks"]))
    pos0, amp0 = ExponentialFP.track_positions(frames, rest, shape_std=sigma, search=search)
    again, _ = ExponentialFP.track_positions(frames, rest, shape_std=sigma, search=search, exclude=0)
    np.testing.assert_array_equal(again, pos0)
    pos, amp = ExponentialFP.track_positions(frames, rest, shape_std=sigma, search=search, exclude=2)
    assert isinstance(pos, np.ndarray) and pos.dtype == np.float64 and pos.shape == truth.shape and amp.shape == truth.shape[::2]
    e15 = TX.pair_errors(dict(positions=pos0), truth)
    err = TX.pair_errors(dict(positions=pos), truth)
    da = np.abs(amp / amps[:, None] - 1).max()
    print(f"pair {TX.PAIRS[pair]}: K15 {e15[0]:.3f} / {e15[1]:.3f}, exclude=2 {err[0]:.3f} / {err[1]:.3f}, amplitude deviation {da:.4f}")
    if pair < 3:
        assert e15[1] > 3.0 and err.max() < 0.5 and da < 0.1
    else:
        assert err[1] < 0.5 * e15[1]


def raw_call(sz, T, K, sigma, search, rounds, guard=5):
    """The C entry itself on zero frames and output buffers filled with -7."""
    from dnmf_amd import _lib
    lib = _lib.load()
    rows = torch.zeros((T, int(np.prod(sz))), device="cuda")
    pred = torch.full((K, 3), 20.0, dtype=torch.float64, device="cuda")
    order = torch.arange(K, dtype=torch.int32, device="cuda")[:, None].repeat(1, T).contiguous()
    pos = torch.full((K * 3 * T,), -7.0, dtype=torch.float64, device="cuda")
    amp = torch.full((K * T,), -7.0, device="cuda")
    peak = torch.full((K * T,), -7.0, device="cuda")
    nsub = torch.full((K * T,), -7, dtype=torch.int32, device="cuda")
    I3 = ctypes.c_int * 3
    rc = lib.dnmf_track_neurons_exclusive(rows.data_ptr(), rows.stride(0), I3(*sz), T, None, pred.data_ptr(), 1, 0, K, order.data_ptr(), rounds,
                                          sigma, I3(*search), 0.0, None, pos.data_ptr(), amp.data_ptr(), peak.data_ptr(), nsub.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    untouched = bool((pos == -7).all() and (amp == -7).all() and (peak == -7).all() and (nsub == -7).all())
    return rc, lib.dnmf_last_error(), untouched


def test_refusals_come_with_a_message_and_before_any_launch():
    from dnmf_amd import _lib, ops
    rc, text, untouched = raw_call((40, 36, 1), 2, 3, 2.0, (4, 4, 0), 0)
    assert rc == -2 and b"rounds" in text and untouched
    rc, text, untouched = raw_call((40, 36, 1), 2, 1025, 2.0, (4, 4, 0), 2)
    assert rc == -3 and b"1024" in text and untouched
    rc, text, untouched = raw_call((64, 64, 4), 2, 3, 8.0, (12, 12, 1), 2)
    assert rc == -3 and b"LDS" in text and untouched
    rc, text, untouched = raw_call((512, 512, 2), 2, 1024, 3.0, (6, 6, 1), 2)          # K15 takes this region; the list does not fit beside it
    assert rc == -3 and b"placed list" in text and untouched
    rc, text, untouched = raw_call((40, 36, 1), 2, 3, 2.0, (4, 4, 0), 2)               # and the same call in bounds runs
    assert rc == 0 and not untouched
    rows = torch.zeros((2, 40 * 36), device="cuda")
    pred = torch.full((3, 3), 20.0, dtype=torch.float64, device="cuda")
    good = torch.tensor([[0, 2], [1, 1], [2, 0]], dtype=torch.int32, device="cuda")
    for bad in (torch.tensor([[0, 2], [1, 1], [1, 0]], dtype=torch.int32, device="cuda"),
                torch.tensor([[0, 2], [1, 1], [3, 0]], dtype=torch.int32, device="cuda"), good.long(), good[:2], good.cpu()):
        with pytest.raises(ValueError, match="order"):
            ops.track_neurons_exclusive(rows, (40, 36, 1), pred, bad, shape_std=2.0, search=(4, 4, 0))
    with pytest.raises(ValueError, match="rounds"):
        ops.track_neurons_exclusive(rows, (40, 36, 1), pred, good, shape_std=2.0, search=(4, 4, 0), rounds=0)
    with pytest.raises(ValueError, match="search"):
        ops.track_neurons_exclusive(rows, (40, 36, 1), pred, good, search=(1, -1, 0))
    many = torch.full((1025, 3), 20.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.DnmfHipError, match="1024"):
        ops.track_neurons_exclusive(rows, (40, 36, 1), many, torch.arange(1025, dtype=torch.int32, device="cuda")[:, None].repeat(1, 2),
                                    shape_std=2.0, search=(4, 4, 0))
    with pytest.raises(_lib.DnmfHipError, match="LDS"):
        ops.track_neurons_exclusive(torch.zeros((2, 64 * 64 * 4), device="cuda"), (64, 64, 4), pred, good, shape_std=8.0, search=(12, 12, 1))
    pos, amp, peak, nsub = ops.track_neurons_exclusive(rows, (40, 36, 1), pred, good, shape_std=2.0, search=(4, 4, 0))
    assert torch.isnan(pos).all() and torch.isnan(amp).all() and (nsub == 0).all()      # a zero frame: no score above the threshold 0
