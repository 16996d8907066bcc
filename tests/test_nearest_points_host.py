"""K10 (dnmf_nearest_points) on the CPU: the workspace formula and every refusal, which must come back with its code and a
text in dnmf_last_error before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def frame_bytes(N):
    """Per-frame workspace: a 256-B header (cell grid, box), 32-B records, (cell, rank) per point, N + 1 cell counts, one sum
    per tile of 1024 counts; rounded up to 256 B."""
    tiles = (N + 1 + 1023) // 1024
    end = 256 + 32 * N + 8 * N + 4 * (N + 1) + 4 * tiles
    return (end + 255) // 256 * 256


def workspace(N, B):
    chunk = min(max(1, (512 << 20) // frame_bytes(N)), 65535, B)
    return chunk * frame_bytes(N)


@pytest.mark.parametrize("N", [1, 2, 3, 1023, 1024, 1025, 4096, 262144, 256 * 256 * 20, (1 << 30) - 1])
@pytest.mark.parametrize("B", [1, 7, 256, 70000])
def test_workspace_formula(lib, N, B):
    assert lib.dnmf_nearest_points_workspace(N, B) == workspace(N, B)
    assert lib.dnmf_nearest_points_workspace(N, B) <= max(512 << 20, frame_bytes(N))


def test_workspace_of_nothing(lib):
    assert lib.dnmf_nearest_points_workspace(0, 4) == 0
    assert lib.dnmf_nearest_points_workspace(-1, 4) == 0
    assert lib.dnmf_nearest_points_workspace(4, 0) == 0
    # a 512x512 frame: 46 frames per 512 MiB chunk
    assert lib.dnmf_nearest_points_workspace(262144, 1000) == 46 * frame_bytes(262144)


def test_refusals_before_any_launch(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 255) // 256 * 256      # 256-aligned, inside the buffer
    big = len(buf) - 256
    N, Q, B = 10, 12, 2

    def call(points=a, f64=0, ldp=3 * N, n=N, queries=a, ldq=3 * Q, q=Q, b=B, values=None, ldv=N, index=a, ldi=Q, vout=None,
             ldo=Q, ws=a, wsb=big):
        return lib.dnmf_nearest_points(points, f64, ldp, n, queries, ldq, q, b, values, ldv, index, ldi, vout, ldo, ws, wsb,
                                       None)

    def refused(rc, code, word):
        assert rc == code, (rc, lib.dnmf_last_error())
        assert word in lib.dnmf_last_error(), lib.dnmf_last_error()

    refused(call(points=None), -1, b"NULL")
    refused(call(queries=None), -1, b"NULL")
    refused(call(index=None), -1, b"NULL")
    refused(call(ws=None), -1, b"NULL")
    refused(call(values=a), -1, b"go together")
    refused(call(vout=a), -1, b"go together")
    refused(call(n=0), -2, b"N=0")
    refused(call(n=-3), -2, b"N=-3")
    refused(call(q=-1), -2, b"Q=-1")
    refused(call(b=-1), -2, b"B=-1")
    refused(call(n=1 << 30, ldp=3 << 30), -3, b"2^30")
    refused(call(ldp=3 * N - 1), -2, b"ldp")
    refused(call(ldq=3 * Q - 1), -2, b"ldq")
    refused(call(ldi=Q - 1), -2, b"ldi")
    refused(call(values=a, vout=a, ldv=N - 1), -2, b"ldv")
    refused(call(values=a, vout=a, ldo=Q - 1), -2, b"ldo")
    one = lib.dnmf_nearest_points_workspace(N, 1)
    refused(call(wsb=one - 1), -4, b"workspace")
    refused(call(ws=a + 16), -4, b"aligned")
    # one query set for every frame, nothing to do: accepted without a launch
    assert call(ldq=0, q=0) == 0
    assert call(b=0) == 0
