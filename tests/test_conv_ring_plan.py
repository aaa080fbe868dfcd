"""csrc/conv1x1_plan.h, conv_nn_ring_rows: the tile height the persistent ring kernel of the channel GEMM runs with (plain C++,
compiled here for the host as tests/test_host_logic.py does with conv_nn_plan)."""
import ctypes
import subprocess

import pytest


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    from makani_amd import build
    d = tmp_path_factory.mktemp("ring_plan")
    src = d / "rows.cpp"
    src.write_text('#include "conv1x1_plan.h"\nextern "C" int rows(int M, int K, int B, long long N, int epi, int env) '
                   '{ return conv_nn_ring_rows(M, K, B, N, epi != 0, env); }\n')
    so = str(d / "rows.so")
    subprocess.check_call([build.HIPCC, "-x", "c++", "-std=c++17", "-shared", "-fPIC", "-I", build.CSRC, str(src), "-o", so])
    L = ctypes.CDLL(so)
    L.rows.argtypes = [ctypes.c_int] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 2

    def f(M, K, N, B=1, epi=False, env=-1):
        return L.rows(M, K, B, N, int(epi), env)
    return f


def test_the_train_step_runs_384_from_768_on_one_384_row_tile(rows):
    """the MLP's second layer (bias) and the data gradient of its first (plain) at the internal and the full resolution"""
    assert rows(384, 768, 115200) == 384 and rows(384, 768, 1038240) == 384


def test_shard_sized_grids_keep_two_192_row_tiles(rows):
    """57 and 127 pixel tiles of 256: fewer 384-row tiles than the persistent grid has workgroups"""
    assert rows(384, 768, 14400) == 192 and rows(384, 768, 32400) == 192


def test_the_tile_count_threshold_is_256_tiles_over_pixels_and_batch(rows):
    assert rows(384, 768, 256 * 255) == 192 and rows(384, 768, 256 * 255 + 8) == 384
    assert rows(384, 768, 256 * 128, B=2) == 384 and rows(384, 768, 256 * 127, B=2) == 192
    assert rows(384, 768, 16 * 40) == 192                                # the dispatch-boundary shape of tests/test_gpu_conv_ring384.py


def test_other_heights_stay(rows):
    """one 192-row tile, whole 256-row tiles, and more than 576 rows run as before at every pixel count"""
    for N in (14400, 115200, 1038240):
        assert [rows(M, 768, N) for M in (192, 256, 677, 768)] == [192, 256, 256, 256], N
    assert rows(193, 768, 115200) == 384 and rows(300, 768, 115200) == 384 and rows(385, 768, 115200) == 192
    assert rows(576, 768, 115200) == 192 and rows(577, 768, 115200) == 256


def test_short_contractions_stay(rows):
    """K = 384 reaches the ring kernel on shards and with two epilogue operands; its tile stays"""
    assert rows(384, 384, 115200) == 192 and rows(384, 448, 115200) == 192 and rows(384, 512, 115200) == 384


def test_every_epilogue_but_plain_and_bias_stays(rows):
    """activation, stored pre-activation, residual and gelu' operands cost the 192-row epilogue another 32 registers: the caller
    passes has_epilogue for any of them (a bias alone is not one)"""
    for N in (14400, 32400, 115200, 1038240):
        assert rows(384, 768, N, epi=True) == 192, N
    assert rows(768, 768, 115200, epi=True) == 256 and rows(300, 1344, 115200, epi=True) == 192


def test_the_override_forces_the_old_tile(rows):
    """MAKANI_AMD_RING384=0"""
    assert rows(384, 768, 115200, env=0) == 192 and rows(384, 768, 1038240, env=0) == 192
    assert rows(384, 768, 115200, env=1) == 384 and rows(384, 768, 14400, env=1) == 192
    assert rows(768, 768, 115200, env=0) == 256
