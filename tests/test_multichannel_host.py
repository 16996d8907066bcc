"""CPU-side checks of the channel entries of K7 and the list-form K5 (dnmf_image_iwarp_channels,
dnmf_spatial_accum_lists_channels): their arguments are validated before any HIP call, so a CPU-only box can exercise them."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


_BUF = ctypes.create_string_buffer(64)   # a host address the entries never dereference: they refuse before any launch


@pytest.fixture(scope="module")
def addr():
    return ctypes.addressof(_BUF)


def test_image_iwarp_channels_validates_its_arguments(lib, addr):
    X, Y, Z, T, B = 8, 6, 1, 4, 2
    P = X * Y * Z
    ws = lib.dnmf_image_iwarp_workspace(X, Y, Z, B)   # the same workspace as one channel: per lattice point, not per channel

    def call(ldf=3 * P, ldc_in=P, nchan=3, ldo=3 * P, ldc_out=P, frames=addr, nbytes=ws):
        return lib.dnmf_image_iwarp_channels(frames, ldf, ldc_in, nchan, None, X, Y, Z, addr, T, addr, B, addr, ldo, ldc_out, addr,
                                             nbytes, 0, None, None)

    assert call(frames=None) == -1 and b"dnmf_image_iwarp_channels: NULL" in lib.dnmf_last_error()
    assert call(nchan=0) == -2 and b"nchan=0" in lib.dnmf_last_error()
    assert call(ldc_in=P - 1) == -2
    assert call(ldc_out=P - 1) == -2
    assert call(ldf=3 * P - 1) == -2 and b"cannot hold 3 channels" in lib.dnmf_last_error()
    assert call(ldo=2 * P + P - 1) == -2
    assert call(ldf=4 * P, ldc_in=P + 1, ldo=3 * P, ldc_out=P + 1) == -2   # the output rows are one float too short
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.dnmf_last_error()
    # one channel: no channel stride is needed (the dnmf_image_iwarp call)
    assert call(nchan=1, ldf=P, ldo=P, ldc_in=0, ldc_out=0, nbytes=ws - 1) == -4
    # and the single-channel entry reports as before
    assert lib.dnmf_image_iwarp(addr, P - 1, None, X, Y, Z, addr, T, addr, B, addr, P, addr, ws, 0, None, None) == -2
    assert b"dnmf_image_iwarp: ldf=" in lib.dnmf_last_error()


def test_spatial_accum_lists_channels_validates_its_arguments(lib, addr):
    X, Y, Z, T, K = 32, 32, 2, 1000, 5
    P = X * Y * Z
    total = 256 * 3 * lib.dnmf_spatial_lists_tiles(X, Y, Z)
    need = lib.dnmf_spatial_accum_lists_workspace(X, Y, Z, total, T)
    assert need > 0   # several splits of the frames at this geometry (the workspace is that of one channel)

    def call(ldy=3 * P, ldyc=P, nchan=3, colours=addr, Yp=addr, ws=addr, nbytes=need):
        return lib.dnmf_spatial_accum_lists_channels(Yp, ldy, ldyc, nchan, colours, None, addr, T, None, T, X, Y, Z, K, addr, total,
                                                     addr, addr, ws, nbytes, None)

    assert call(Yp=None) == -1 and b"dnmf_spatial_accum_lists_channels: NULL" in lib.dnmf_last_error()
    assert call(colours=None) == -1 and b"colours" in lib.dnmf_last_error()
    assert call(nchan=0) == -2
    assert call(ldyc=P - 1) == -2
    assert call(ldy=3 * P - 1) == -2
    assert call(nbytes=need - 4) == -4 and b"workspace" in lib.dnmf_last_error()
    assert call(ws=None, nbytes=0) == -4
    # one channel without colours is the single-channel call; with colours it is checked like any other
    assert call(nchan=1, ldy=P, ldyc=0, colours=None, nbytes=need - 4) == -4
    assert lib.dnmf_spatial_accum_lists(addr, P - 1, None, addr, T, None, T, X, Y, Z, K, addr, total, addr, addr, None, 0, None) == -2
    assert b"dnmf_spatial_accum_lists: T=" in lib.dnmf_last_error()
