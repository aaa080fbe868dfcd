"""The block tail ``outer_skip(residual) + norm1(z [+ pb])`` as one statistics pass and one GEMM (``ops.SkipNormFn``:
``mk_instnorm_stats_fused`` + ``mk_conv1x1_nn_rnorm``) against the two-step path it replaces (``InstanceNormFn`` followed by
``Conv1x1Fn(residual=y)``): the fold must not change a bit — output, statistics and all five gradients are compared with
``torch.equal``.

Shapes (C = 384, bf16): 131 x 264 = 34 584 pixels — above the 32 768 below which 384 <- 384 plans the ring kernel, 34 584 % 64 = 24
(a ragged last pixel tile), % 8 = 0 — and 128 x 264 = 33 792 (whole tiles); B = 1, 2; with and without the deferred fc2 bias;
random gamma / beta.  Each case is 13 - 27 M elements: a fraction of a second."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 384
EPS = 1e-6


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _case(B, H, W, with_pb, seed):
    g = torch.Generator().manual_seed(seed)
    dev = _dev()
    res = torch.randn(B, C, H, W, generator=g).bfloat16().to(dev)
    # planes with their own offset and spread, so that mean and rstd differ from plane to plane
    z = (torch.randn(B, C, H, W, generator=g) * (0.5 + torch.rand(B, C, 1, 1, generator=g) * 2) + torch.randn(B, C, 1, 1, generator=g)).bfloat16().to(dev)
    weight = (torch.randn(C, C, 1, 1, generator=g) / math.sqrt(C)).to(dev)
    gamma = (1 + 0.5 * torch.randn(C, generator=g)).to(dev)
    beta = (0.3 * torch.randn(C, generator=g)).to(dev)
    pb = (0.2 * torch.randn(C, generator=g)).to(dev) if with_pb else None
    cot = torch.randn(B, C, H, W, generator=g).bfloat16().to(dev)
    return res, z, weight, gamma, beta, pb, cot


def _run(fold, res, z, weight, gamma, beta, pb, cot):
    """(output, gradients of res, z, weight, gamma, beta) of one forward + backward on fresh leaves"""
    from makani_amd import ops
    leaves = [t.clone().requires_grad_(True) for t in (res, z, weight, gamma, beta)]
    r, zz, w, ga, be = leaves
    if fold:
        out = ops.SkipNormFn.apply(r, w, zz, ga, be, EPS, pb)
    else:
        y = ops.InstanceNormFn.apply(zz, ga, be, EPS, False, pb)
        out = ops.Conv1x1Fn.apply(r, w, None, y)
    out.backward(cot)
    torch.cuda.synchronize()
    return [out.detach()] + [t.grad for t in leaves]


def _stats(z, gamma, beta, pb):
    """(mean, rstd) per plane as mk_instnorm_fwd_fused and as mk_instnorm_stats_fused write them"""
    from makani_amd import ops
    from makani_amd._lib import check, dtype_code, lib, ptr, stream
    B, Cc, H, W = z.shape
    planes, hw = B * Cc, H * W
    ch = int(lib().mk_instnorm_fused_chunks(hw, dtype_code(z), planes, 0))
    assert ch > 0
    g, b = gamma.float().contiguous(), beta.float().contiguous()
    p = pb.float().contiguous() if pb is not None else None
    y = torch.empty_like(z)
    st_a = torch.empty((planes, 2), dtype=torch.float32, device=z.device)
    slots, depart = ops._fused_sync(planes * ch, planes, z.device)
    check(lib().mk_instnorm_fwd_fused(ptr(z), ptr(y), dtype_code(z), ptr(st_a), ptr(g), ptr(b), ptr(p), ptr(slots), ptr(depart), planes, Cc,
                                      hw, EPS, 0, stream()), "instnorm_fwd_fused")
    st_b = torch.empty((planes, 2), dtype=torch.float32, device=z.device)
    coef = torch.empty(((planes + 7) // 8 * 8, 2), dtype=torch.float32, device=z.device)
    ws = torch.empty((planes * ch * 2,), dtype=torch.float32, device=z.device)
    check(lib().mk_instnorm_stats_fused(ptr(z), dtype_code(z), ptr(st_b), ptr(coef), ptr(ws), ptr(g), ptr(b), ptr(p), planes, Cc, hw, EPS,
                                        stream()), "instnorm_stats_fused")
    torch.cuda.synchronize()
    return st_a, st_b


@pytest.mark.parametrize("with_pb", [False, True])
@pytest.mark.parametrize("H,W", [(131, 264), (128, 264)])
@pytest.mark.parametrize("B", [1, 2])
def test_fold_equals_norm_then_skip_gemm_bit_for_bit(B, H, W, with_pb):
    from makani_amd import layers, ops
    res, z, weight, gamma, beta, pb, cot = _case(B, H, W, with_pb, seed=1000 * B + H + int(with_pb))
    assert ops.skip_norm_fold_supported(res, weight, z)
    want = _run(False, res, z, weight, gamma, beta, pb, cot)
    got = _run(True, res, z, weight, gamma, beta, pb, cot)
    assert torch.isfinite(want[0].float()).all() and want[0].float().abs().max() > 1
    for name, a, b in zip(("out", "grad res", "grad z", "grad weight", "grad gamma", "grad beta"), got, want):
        assert a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
    st_a, st_b = _stats(z, gamma, beta, pb)
    assert torch.equal(st_a, st_b), (st_a - st_b).abs().max().item()
    # the layer-level dispatch picks the fold for these shapes
    conv = layers.PointwiseConv(C, C, bias=False).to(_dev())
    norm = layers.InstanceNorm2d(C, eps=EPS, affine=True).to(_dev())
    assert layers.skip_norm_foldable(conv, norm, res, z)


def test_fold_is_repeatable_eagerly_and_under_graph_replay():
    from makani_amd import ops
    res, z, weight, gamma, beta, pb, cot = _case(1, 131, 264, True, seed=77)
    want = _run(False, res, z, weight, gamma, beta, pb, cot)
    for _ in range(3):                                  # back to back: nothing of one call survives into the next
        got = _run(True, res, z, weight, gamma, beta, pb, cot)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.SkipNormFn.apply(res, weight, z, gamma, beta, EPS, pb)          # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.SkipNormFn.apply(res, weight, z, gamma, beta, EPS, pb)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[0])


def test_shard_sized_grid_keeps_the_two_step_path():
    """14 400 pixels: 384 <- 384 plans the ring kernel, which has no normalising operand — the dispatch says no, the C entry
    refuses the shape (an error, not another kernel), and the block tail is the two-step result it always was"""
    from makani_amd import layers, ops
    from makani_amd._lib import lib, ptr, stream
    res, z, weight, gamma, beta, pb, cot = _case(1, 120, 120, True, seed=5)
    assert not ops.skip_norm_fold_supported(res, weight, z)
    conv = layers.PointwiseConv(C, C, bias=False).to(_dev())
    norm = layers.InstanceNorm2d(C, eps=EPS, affine=True).to(_dev())
    with torch.no_grad():
        conv.weight.copy_(weight)
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    assert not layers.skip_norm_foldable(conv, norm, res, z)
    want = _run(False, res, z, weight, gamma, beta, pb, cot)
    with torch.no_grad():
        out = conv(res, add_to=norm(z, pre_bias=pb), add_to_is_fresh=True)
    assert torch.equal(out, want[0])
    A = ops.pad_weight_bf16(weight.view(C, C))
    coef = torch.zeros((C, 2), dtype=torch.float32, device=_dev())
    y = torch.empty_like(z)
    rc = lib().mk_conv1x1_nn_rnorm(ptr(A), ptr(res), ptr(y), ptr(None), ptr(None), ptr(z), ptr(None), C, C, C, 1, 14400, 0, ptr(coef),
                                   ptr(None), C, stream())
    assert rc != 0
