"""``ops._boxes``, the one place where the box kernels' callers (K24 ``component_stats``, K26 ``component_pairs``, K27
``clean_footprints``, K28a ``residual_boxes``) turn ``boxes`` into what the library takes: the host int32 copy, the device copy
and the voxel counts, and the messages of its refusals word for word.  Pure torch on the CPU: no library, no GPU."""
import pytest
import torch

from dnmf_amd import ops

SZ = (8, 6, 2)
GOOD = [0, 3, 0, 3, 0, 1]                                  # 4 x 4 x 2 = 32 voxels
BAD = {"a negative corner": [-1, 3, 0, 3, 0, 1], "a corner at S": [0, 8, 0, 3, 0, 1], "lo > hi": [5, 4, 0, 3, 0, 1]}


def check_triple(got, boxes, nvox):
    bh, bd, n = got
    assert bh.dtype == torch.int32 and bh.device.type == "cpu" and bh.is_contiguous() and bh.tolist() == boxes
    assert bd.dtype == torch.int32 and bd.tolist() == boxes
    assert n.dtype == torch.int64 and n.tolist() == nvox


def test_a_good_box_as_tensor_and_as_nested_ints():
    boxes = [GOOD, [7, 7, 5, 5, 1, 1], [0, 7, 0, 5, 0, 1]]  # the last: the whole volume, corners at S - 1
    for given in (boxes, torch.tensor(boxes), torch.tensor(boxes, dtype=torch.int64), torch.tensor(boxes, dtype=torch.float64)):
        check_triple(ops._boxes("fn", given, SZ), boxes, [32, 1, 96])
        check_triple(ops._boxes("fn", given, SZ, 3, dev="cpu"), boxes, [32, 1, 96])
    check_triple(ops._boxes("fn", [GOOD], torch.tensor(SZ)), [GOOD], [32])
    # exactly the limit passes, and a limit of the caller's own is the one compared against
    check_triple(ops._boxes("fn", [[0, 15, 0, 15, 0, 15]], (16, 16, 16)), [[0, 15, 0, 15, 0, 15]], [4096])
    check_triple(ops._boxes("fn", [GOOD], SZ, limit=32), [GOOD], [32])
    with pytest.raises(ValueError) as e:
        ops._boxes("fn", [GOOD], SZ, limit=31)
    assert str(e.value) == "fn: box 0 holds 32 voxels, at most 31"


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_box_that_is_empty_or_outside(name):
    bad = BAD[name]
    for fn, kw in (("clean_footprints", dict(n=2, noun="the box of neuron")), ("residual_boxes", {})):
        with pytest.raises(ValueError) as e:
            ops._boxes(fn, [GOOD, bad], SZ, **kw)
        assert str(e.value) == f"{fn}: box 1 = {bad} is empty or outside the volume 8x6x2"
    # the first wrong box is the one named
    with pytest.raises(ValueError) as e:
        ops._boxes("fn", [bad, GOOD, BAD["lo > hi"]], SZ)
    assert str(e.value) == f"fn: box 0 = {bad} is empty or outside the volume 8x6x2"
    # component_stats and component_pairs leave the judgement to the library: the copies and the counts come back as they are
    bh, bd, n = ops._boxes("component_stats", [GOOD, bad], SZ, 2, check=False)
    assert bh.tolist() == [GOOD, bad] and bd.tolist() == [GOOD, bad] and n[0] == 32


def test_a_box_of_4097_voxels():
    sz, big = (17, 241, 1), [0, 16, 0, 240, 0, 0]
    with pytest.raises(ValueError) as e:
        ops._boxes("residual_boxes", [[0, 0, 0, 0, 0, 0], big], sz)
    assert str(e.value) == "residual_boxes: box 1 holds 4097 voxels, at most 4096"
    with pytest.raises(ValueError) as e:
        ops._boxes("clean_footprints", torch.tensor([[0, 0, 0, 0, 0, 0], big]), sz, 2, noun="the box of neuron")
    assert str(e.value) == "clean_footprints: the box of neuron 1 holds 4097 voxels, at most 4096"
    # outside the volume is said before too large
    with pytest.raises(ValueError) as e:
        ops._boxes("fn", [big], (17, 240, 1))
    assert str(e.value) == f"fn: box 0 = {big} is empty or outside the volume 17x240x1"
    check_triple(ops._boxes("fn", [big], sz, check=False), [big], [4097])


def test_a_wrong_shape():
    for given, n, text in (([GOOD], 2, "fn: boxes must be (2, 6), got (1, 6)"),
                           ([GOOD[:5], GOOD[:5]], 2, "fn: boxes must be (2, 6), got (2, 5)"),
                           (GOOD, 1, "fn: boxes must be (1, 6), got (6,)"),
                           (GOOD, None, "fn: boxes must be (M, 6), got (6,)"),
                           (torch.zeros((0, 6)), None, "fn: boxes must be (M, 6), got (0, 6)"),
                           ([[GOOD]], None, "fn: boxes must be (M, 6), got (1, 1, 6)"),
                           ([GOOD + [0]], None, "fn: boxes must be (M, 6), got (1, 7)")):
        for check in (True, False):
            with pytest.raises(ValueError) as e:
                ops._boxes("fn", given, SZ, n, check=check)
            assert str(e.value) == text
