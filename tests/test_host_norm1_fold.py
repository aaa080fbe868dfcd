"""Host logic of the norm1 fold (no GPU): ``conv_nn_rnorm_supported`` of csrc/conv1x1_plan.h — the predicate behind
``mk_conv1x1_nn_rnorm_supported`` — is true exactly where ``conv_nn_plan`` puts a call with a residual operand on the two-group
weight-stationary kernel, over the channel GEMMs of the networks, full grids and the shards of one rank, under every setting of
MAKANI_AMD_ASTAT2."""
import ctypes
import subprocess

import pytest


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    from makani_amd import build
    d = tmp_path_factory.mktemp("norm1_fold_plan")
    src = d / "plan.cpp"
    src.write_text('#include "conv1x1_plan.h"\n'
                   'extern "C" int plan(int M, int K, int lda, int B, long long N, int pre, int r, int g, int a2) '
                   '{ return (int)conv_nn_plan(M, K, lda, B, N, pre, r, g, a2); }\n'
                   'extern "C" int rnorm(int M, int K, int lda, int B, long long N, int a2) '
                   '{ return conv_nn_rnorm_supported(M, K, lda, B, N, a2) ? 1 : 0; }\n')
    so = str(d / "plan.so")
    subprocess.check_call([build.HIPCC, "-x", "c++", "-std=c++17", "-shared", "-fPIC", "-I", build.CSRC, str(src), "-o", so])
    L = ctypes.CDLL(so)
    L.plan.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong] + [ctypes.c_int] * 4
    L.rnorm.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong] + [ctypes.c_int]
    return L


ASTAT2 = 1      # ConvNnKernel::astat2
FULL = (115200, 1038240, 34584, 33792)                  # the flagship's two grids, the two sizes of the GPU test
SHARD = (14400, 32400, 32768)                           # one rank of h4 w2 ... the largest grid that still plans the ring kernel
SHAPES = [(384, 384, 384), (768, 384, 384), (384, 768, 768), (384, 73, 80), (73, 384, 384), (256, 384, 384), (400, 384, 384),
          (128, 384, 384), (1536, 384, 384)]


def test_rnorm_supported_is_the_plan_of_a_call_with_a_residual_operand(plan_lib):
    L = plan_lib
    for a2 in (-1, 0, 1):
        for (M, K, lda) in SHAPES:
            for B in (1, 2):
                for N in FULL + SHARD:
                    want = L.plan(M, K, lda, B, N, 0, 1, 0, a2) == ASTAT2
                    assert bool(L.rnorm(M, K, lda, B, N, a2)) == want, (M, K, lda, B, N, a2)


def test_rnorm_supported_on_the_block_tail_of_the_networks(plan_lib):
    L = plan_lib
    for B in (1, 2):
        for N in FULL:                                  # the skip GEMM 384 <- 384 of every block on a full grid: folded
            assert L.rnorm(384, 384, 384, B, N, -1) == 1, (B, N)
    for N in SHARD:                                     # shard-sized grids plan the ring kernel: the two-step path
        assert L.rnorm(384, 384, 384, 1, N, -1) == 0, N
        assert L.rnorm(384, 384, 384, 1, N, 1) == 1, N  # ... unless the two-group kernel is forced onto them
    assert L.rnorm(384, 384, 384, 2, 14400, -1) == 0 and L.rnorm(384, 384, 384, 2, 32400, -1) == 1      # (the threshold counts B N)
    for N in FULL:
        assert L.rnorm(384, 384, 384, 1, N, 0) == 0     # MAKANI_AMD_ASTAT2=0: the one-group kernel has no normalising operand
        assert L.rnorm(384, 768, 768, 1, N, -1) == 0 and L.rnorm(384, 73, 80, 1, N, -1) == 0 and L.rnorm(73, 384, 384, 1, N, -1) == 0
        assert L.rnorm(1536, 384, 384, 1, 1038240, -1) == 0          # byte offsets of a batch entry past 32 bits
