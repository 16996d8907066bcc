"""What the four entries that take per-component boxes raise for a bad one: K24 ``ops.component_stats`` and K26
``ops.component_pairs`` leave the judgement to the library (``DnmfHipError`` with its text, from the workspace entry and from
the call's ``DNMF_E_SHAPE``), K27 ``ops.clean_footprints`` and K28a ``ops.residual_boxes`` refuse in Python (``ValueError``, the
box as a list).  The entries share their box handling (``ops._boxes``, csrc/boxes.hpp); these differences are kept on purpose and
pinned here, type and text.  8 x 6 x 2 voxels, K = 2, T = 4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SZ, K, T = (8, 6, 2), 2, 4
P = SZ[0] * SZ[1] * SZ[2]
GOOD = [0, 3, 0, 3, 0, 1]
# the bad box -> how the library prints it
BAD = {"a negative corner": ([-1, 3, 0, 3, 0, 1], "x -1..3, y 0..3, z 0..1"),
       "a corner at S": ([0, 8, 0, 3, 0, 1], "x 0..8, y 0..3, z 0..1"),
       "lo > hi": ([5, 4, 0, 3, 0, 1], "x 5..4, y 0..3, z 0..1")}
OUTSIDE = "is empty or outside the volume 8x6x2"


@pytest.fixture(scope="module")
def entries():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import _lib, ops
    g = torch.Generator().manual_seed(0)
    frames = torch.rand((T, P), generator=g).cuda()
    A_rows = torch.rand((K, P), generator=g).cuda()
    A = A_rows.t().contiguous()
    C = torch.rand((K, T), generator=g).cuda()
    w = torch.ones((K, T), device="cuda")
    return _lib.DnmfHipError, {
        "component_stats": lambda boxes: ops.component_stats(frames, SZ, A_rows, boxes, C, w),
        "component_pairs": lambda boxes: ops.component_pairs(A_rows, SZ, boxes, C),
        "clean_footprints": lambda boxes: ops.clean_footprints(A, SZ, boxes),
        "residual_boxes": lambda boxes: ops.residual_boxes(frames, SZ, boxes),
    }


def test_good_boxes_pass(entries):
    for call in entries[1].values():
        call([GOOD, [4, 7, 2, 5, 0, 1]])
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_bad_box(entries, name):
    DnmfHipError, calls = entries
    bad, printed = BAD[name]
    expected = {
        "component_stats": (DnmfHipError, "dnmf_component_stats_workspace refused: dnmf_component_stats_workspace: box 1 = "
                                          f"{printed} {OUTSIDE}"),
        "component_pairs": (DnmfHipError, "dnmf_component_pairs failed (argument error -2): dnmf_component_pairs: box 1 = "
                                          f"{printed} {OUTSIDE}"),
        "clean_footprints": (ValueError, f"clean_footprints: box 1 = {bad} {OUTSIDE}"),
        "residual_boxes": (ValueError, f"residual_boxes: box 1 = {bad} {OUTSIDE}"),
    }
    for entry, call in calls.items():
        kind, text = expected[entry]
        for boxes in ([GOOD, bad], torch.tensor([GOOD, bad], dtype=torch.int32, device="cuda")):
            with pytest.raises(Exception) as e:
                call(boxes)
            assert type(e.value) is kind and str(e.value) == text, (entry, type(e.value), str(e.value))
