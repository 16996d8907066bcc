"""The rule "the neuron-list kernel forms apply" (``dNMF.lists_verdict``) and the cache of packed footprint layouts, on
the host: no GPU, no library."""
import copy

import pytest
import torch

from dnmf_amd import ops
from dnmf_amd.Demix import dNMF
from dnmf_amd.Demix.dNMF import ExponentialFP, lists_verdict

# What each call site of the driver asks the rule, written from the conditions the five sites spelled out before they
# shared it.  (site, mode, K, boxfrac, nslot, nbr exists) -> the lists apply
LIM, SLOTS = 6.0, 3800
TABLE = [
    # recon_image / _motion_lists_layout: K <= 256 and boxfrac < limit; nslot and nbr are not looked at
    ("recon", "auto", 100, 2.0, 99999, False, True),
    ("recon", "auto", 256, 5.99, 1, True, True),
    ("recon", "auto", 257, 1.0, 1, True, False),
    ("recon", "auto", 100, 6.0, 1, True, False),
    ("recon", "auto", 100, 7.5, 1, True, False),
    # _gram_rhs_one: mode in (auto, lists), K <= 256, nslot <= 3800, 'lists' or boxfrac < limit; nbr not looked at
    ("gram", "auto", 100, 2.0, 3800, False, True),
    ("gram", "auto", 100, 2.0, 3801, True, False),
    ("gram", "auto", 100, 6.0, 100, True, False),
    ("gram", "auto", 256, 5.0, 100, True, True),
    ("gram", "auto", 257, 5.0, 100, True, False),
    ("gram", "lists", 100, 6.0, 3800, False, True),
    ("gram", "lists", 100, 50.0, 100, True, True),
    ("gram", "lists", 100, 1.0, 3801, True, False),
    ("gram", "lists", 257, 1.0, 100, True, False),
    ("gram", "dense", 100, 1.0, 100, True, False),
    ("gram", "sparse", 100, 1.0, 100, True, False),
    ("gram", "bf16", 100, 1.0, 100, True, False),
    # _lists_layout_for_fused_update: as gram, and nbr exists
    ("fused", "auto", 100, 2.0, 3800, True, True),
    ("fused", "auto", 100, 2.0, 3800, False, False),
    ("fused", "auto", 100, 2.0, 3801, True, False),
    ("fused", "auto", 100, 6.0, 100, True, False),
    ("fused", "auto", 257, 2.0, 100, True, False),
    ("fused", "lists", 100, 9.0, 3800, True, True),
    ("fused", "lists", 100, 9.0, 3800, False, False),
    ("fused", "lists", 100, 1.0, 3801, True, False),
    ("fused", "dense", 100, 1.0, 100, True, False),
    # _spatial_lists: mode in (auto, lists), K <= 256, 'lists' or boxfrac < limit; nslot and nbr are not looked at
    ("spatial", "auto", 256, 5.0, 99999, False, True),
    ("spatial", "auto", 257, 5.0, 1, True, False),
    ("spatial", "auto", 100, 6.0, 1, True, False),
    ("spatial", "lists", 100, 6.0, 99999, False, True),
    ("spatial", "lists", 257, 1.0, 1, True, False),
    ("spatial", "dense", 100, 1.0, 1, True, False),
]
ASKS = {"recon": (False, False), "spatial": (False, False), "gram": (True, False), "fused": (True, True)}   # (slots, nbr)


def test_the_limits_are_the_ones_the_table_was_written_for():
    assert (dNMF.LISTS_BOXFRAC_LIMIT, dNMF.LISTS_MAX_K, ops.LISTS_MAX_SLOTS) == (LIM, 256, SLOTS)


@pytest.mark.parametrize("site,mode,K,boxfrac,nslot,has_nbr,applies", TABLE)
def test_lists_verdict_against_the_call_sites(site, mode, K, boxfrac, nslot, has_nbr, applies):
    slots, nbr = ASKS[site]
    why = lists_verdict(mode, K, boxfrac, nslot if slots else None, has_nbr if nbr else None)
    assert (why is None) == applies, why


def test_reasons_that_the_gram_path_acts_on():
    """'auto' prints one note for K and another for the shape; 'lists' raises on the slots only."""
    assert lists_verdict("auto", 257, 1.0, 1) == "K"
    assert lists_verdict("auto", 100, 1.0, SLOTS + 1) == "slots"
    assert lists_verdict("auto", 100, LIM, SLOTS) == "boxes"
    assert lists_verdict("lists", 100, 99.0, SLOTS + 1) == "slots"
    assert lists_verdict("lists", 257, 1.0, SLOTS + 1) == "K"
    assert lists_verdict("dense", 257) == "mode"
    # before a layout exists only the mode and K are known
    assert lists_verdict("auto", 256) is None and lists_verdict("auto", 257) == "K"


def _host_model(monkeypatch, K=3):
    """An ExponentialFP without a GPU: the attributes the layout cache reads, and a counting stand-in for the packing."""
    fp = ExponentialFP.__new__(ExponentialFP)
    torch.nn.Module.__init__(fp)
    fp.sz_list, fp.K, fp.P = [4, 4, 1], K, 16
    fp.A = torch.ones(4, 4, 1, K)
    fp.invalidate_layouts()
    made = []

    def pack(A, sz):
        made.append(A.clone())
        return {"boxfrac": 1.0, "nslot": 5, "nbr": None, "n": len(made)}

    monkeypatch.setattr(ops, "pack_footprints_lists", pack)
    return fp, made


def test_layout_cache_identity_and_invalidation(monkeypatch):
    fp, made = _host_model(monkeypatch)
    ly = fp.packed_lists()
    assert fp.packed_lists() is ly and fp.packed_lists(floor=0.0) is ly and len(made) == 1   # one layout at floor 0
    fp.A.mul_(2.0)                                  # an edit torch sees
    ly2 = fp.packed_lists()
    assert ly2 is not ly and fp.packed_lists() is ly2 and len(made) == 2
    fp.invalidate_layouts()                         # an edit torch does not see (K6 through the raw pointer)
    assert fp.packed_lists() is not ly2 and len(made) == 3
    fp.A = fp.A.clone()                             # a new tensor
    assert fp.packed_lists()["n"] == 4


def test_layout_cache_keeps_the_own_floor_and_floor_zero(monkeypatch):
    fp, made = _host_model(monkeypatch)
    fp.A[0, 0, 0, 0] = 0.25
    fp.footprint_floor = 0.5
    own, exact = fp.packed_lists(), fp.packed_lists(floor=0.0)
    assert own is not exact and len(made) == 2
    assert made[0][0, 0, 0, 0] == 0 and made[1][0, 0, 0, 0] == 0.25     # the floored copy and the true values
    for _ in range(2):                              # they alternate within a sweep: neither evicts the other
        assert fp.packed_lists() is own and fp.packed_lists(floor=0.0) is exact
    assert len(made) == 2


def test_a_shallow_copy_gets_a_cache_of_its_own(monkeypatch):
    fp, made = _host_model(monkeypatch)
    ly = fp.packed_lists()
    f = copy.copy(fp)
    f.A = fp.A * 2.0
    f.invalidate_layouts()
    assert f.packed_lists() is not ly
    assert fp.packed_lists() is ly                  # the copy's layouts did not land in the original's cache
    assert len(made) == 2


def test_model_asks_the_rule_and_builds_no_layout_it_cannot_use(monkeypatch):
    fp, made = _host_model(monkeypatch, K=257)
    assert fp._lists_verdict("auto") == (None, "K") and fp.lists_layout() is None and not made
    fp, made = _host_model(monkeypatch)
    assert fp._lists_verdict("dense") == (None, "mode") and not made
    ly = fp.lists_layout()
    assert ly is fp.packed_lists() and fp.lists_layout(forced=True) is ly
    assert fp._lists_verdict("auto", slots=True) == (ly, None)
    assert fp._lists_verdict("auto", slots=True, nbr=True) == (ly, "nbr")      # the stand-in layout has no column lists
    ly["boxfrac"] = LIM
    assert fp.lists_layout() is None and fp.lists_layout(forced=True) is ly
