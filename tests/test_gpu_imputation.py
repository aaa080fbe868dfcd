"""``mk_impute_mlp_fwd`` / ``_bwd`` and ``mk_impute_const_fwd`` / ``_bwd`` on the GPU, through ``MLPImputation`` and
``ConstantImputation``, against the fp64 restatement of tests/_impute_ref.py (pinned to the reference's recorded values by
tests/test_imputation.py).

Gates, none taken from the code under test.  f32 tensors: with e_t the largest error of the reference's composition evaluated in
fp32 torch on the same inputs against fp64, the kernel's largest error is at most 2 e_t + 4 2^-23 max|ref|, per output tensor and
per gradient tensor (both are fp32 sums of C terms in different orders; the floor is for the cases where e_t is 0).  bf16 tensors:
|y - ref| <= 2^-8 |ref| + 2^-23 max|ref| element by element (fp32 arithmetic, rounded once), the restatement evaluated on the
bf16-rounded inputs; the weight gradients of a bf16 run are f32 tensors and take the f32 gate.  Every figure is printed before it
is asserted.  Invariants, exact: unmasked entries and copied channels are the input bit for bit, the input gradient is a finite 0
at masked entries, a second run repeats the first bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _impute_ref as ref          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
ACT = {"gelu": nn.GELU, "relu": nn.ReLU, "silu": nn.SiLU}


def _act(name):
    from makani_amd.imputation import Sin
    return Sin if name == "sin" else ACT[name]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _offset_view(t):
    """the same values in a contiguous view at storage offset 1: its pointer is not 16-byte aligned"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def make_case(shape, imp, mask, dtype, hidden_ratio, masked="mixed", misaligned=False, mask_channel=None, seed=0):
    """inputs of one case on the CPU in fp32 (already rounded to `dtype`), NaN in the imputed channels included"""
    gen = torch.Generator().manual_seed(1000 + seed)
    *lead, C, H, W = shape
    B = int(np.prod(lead)) if lead else 1
    NI, hidden = len(imp), int(hidden_ratio * len(imp))
    x = torch.randn(B, C, H, W, generator=gen)
    g = torch.randn(B, C, H, W, generator=gen)
    m = None
    if mask_channel is not None:          # a fractional land mask among the channels: 0 over 60 % of the pixels, (0, 1] elsewhere
        u = torch.rand(B, H, W, generator=gen)
        x[:, mask_channel] = torch.where(u < 0.6, torch.zeros(()), (u - 0.6) / 0.4)
    x, g = x.to(dtype).float(), g.to(dtype).float()
    if mask == "bool_ni":
        m = torch.rand(B, NI, H, W, generator=gen) < 0.3
    elif mask == "bool_1":
        m = torch.rand(B, 1, H, W, generator=gen) < 0.3
    if masked == "mixed":
        nan = torch.rand(B, NI, H, W, generator=gen) < 0.2
        x[:, imp] = torch.where(nan, torch.full((), float("nan")), x[:, imp])
    elif masked == "all":
        m = torch.ones(B, NI, H, W, dtype=torch.bool)
    w1 = torch.randn(hidden, C, generator=gen) * (2.0 / C) ** 0.5
    b1 = torch.randn(hidden, generator=gen) * 0.1
    w2 = torch.randn(NI, hidden, generator=gen) * (1.0 / hidden) ** 0.5
    return dict(x=x, g=g, m=m, w1=w1, b1=b1, w2=w2, lead=lead, imp=list(imp), mask_channel=mask_channel, dtype=dtype, misaligned=misaligned)


def module_of(c, act):
    from makani_amd.imputation import MLPImputation
    C, NI, hidden = c["w1"].shape[1], len(c["imp"]), c["w1"].shape[0]
    mod = MLPImputation(C, torch.tensor(c["imp"]), hidden / NI, _act(act), mask_channel=c["mask_channel"]).to(DEV)
    with torch.no_grad():
        mod.mlp.fwd[0].weight.copy_(c["w1"].view(hidden, C, 1, 1))
        mod.mlp.fwd[0].bias.copy_(c["b1"])
        mod.mlp.fwd[2].weight.copy_(c["w2"].view(NI, hidden, 1, 1))
    return mod


def run_module(mod, c):
    """(y, gx, gw1, gb1, gw2) of one forward and backward pass, in the tensors' own dtypes"""
    shape = (*c["lead"], *c["x"].shape[1:])
    x = c["x"].to(DEV, c["dtype"]).view(shape)
    g = c["g"].to(DEV, c["dtype"]).view(shape)
    if c["misaligned"]:
        x, g = _offset_view(x), _offset_view(g)
    x.requires_grad_(True)
    m = None if c["m"] is None else c["m"].to(DEV).view(*c["lead"], *c["m"].shape[1:])
    y = mod(x, m)
    assert y.dtype == c["dtype"] and y.shape == x.shape
    p = [mod.mlp.fwd[0].weight, mod.mlp.fwd[0].bias, mod.mlp.fwd[2].weight]
    gx, gw1, gb1, gw2 = torch.autograd.grad(y, [x] + p, g)
    B = c["x"].shape[0]
    return (y.detach().reshape(B, *shape[-3:]), gx.reshape(B, *shape[-3:]), gw1.reshape(c["w1"].shape), gb1, gw2.reshape(c["w2"].shape))


def references(c, act):
    """the fp64 restatement and the reference's composition in fp32 torch on the GPU, each (y, gx, gw1, gb1, gw2) as fp64 numpy"""
    mask = None if c["m"] is None else c["m"].numpy()
    if c["mask_channel"] is not None:
        mask = (c["x"][:, c["mask_channel"]] != 0).numpy()[:, None]
    a = (c["imp"], mask, c["w1"].numpy(), c["b1"].numpy(), c["w2"].numpy(), act)
    want = (ref.mlp_fwd(c["x"].numpy(), *a), *ref.mlp_bwd(c["x"].numpy(), c["g"].numpy(), *a))
    x = c["x"].to(DEV).requires_grad_(True)
    w = [c[k].to(DEV).requires_grad_(True) for k in ("w1", "b1", "w2")]
    y = ref.compose_mlp(x, c["imp"], None if mask is None else torch.from_numpy(mask).to(DEV), *w, act)
    grads = torch.autograd.grad(y, [x] + w, c["g"].to(DEV))
    return want, [t.detach().double().cpu().numpy() for t in (y, *grads)]


def _err(a, b):
    """the largest |a - b|; a NaN on one side only counts as infinite"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    if (nan_a != nan_b).any():
        return float("inf")
    d = np.abs(np.where(nan_a, 0.0, a) - np.where(nan_b, 0.0, b))
    return float(d.max()) if d.size else 0.0


def gate_f32(name, got, want, torch32):
    e_k, e_t, top = _err(got, want), _err(torch32, want), float(np.nanmax(np.abs(want)))
    bound = 2.0 * e_t + 4.0 * 2.0 ** -23 * top
    print(f"  {name}: kernel {e_k:.3e}  fp32 torch {e_t:.3e}  max|ref| {top:.3e}  bound {bound:.3e}")
    assert e_k <= bound, (name, e_k, e_t, bound)


def gate_bf16(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    top = float(np.abs(want).max())
    excess = np.abs(got - want) - (2.0 ** -8 * np.abs(want) + 2.0 ** -23 * top)
    print(f"  {name}: largest |got - ref| {np.abs(got - want).max():.3e}  max|ref| {top:.3e}  largest excess over the bound {excess.max():.3e}")
    assert excess.max() <= 0.0, (name, float(excess.max()))


def check_case(c, act, expect="mixed"):
    mod = module_of(c, act)
    out = run_module(mod, c)
    again = run_module(mod, c)
    for a, b in zip(out, again):
        assert torch.equal(_bits(a), _bits(b)), "a second run differs"
    y, gx, gw1, gb1, gw2 = out
    want, t32 = references(c, act)
    m = torch.from_numpy(ref.mlp_mask(c["x"].numpy(), c["imp"], None if c["m"] is None else c["m"].numpy()))
    if c["mask_channel"] is not None:
        m = m | (c["x"][:, c["mask_channel"]] != 0)[:, None]
    if expect == "mixed":
        assert m.any() and not m.all(), "the case must hold masked and unmasked entries"
    full = torch.zeros(c["x"].shape, dtype=torch.bool)
    full[:, c["imp"]] = m
    xd = c["x"].to(DEV, c["dtype"])
    # exact: what is not masked is the input bit for bit; the input gradient is a finite zero at masked entries
    assert torch.equal(_bits(y)[~full.to(DEV)], _bits(xd)[~full.to(DEV)])
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    assert (gx[full.to(DEV)] == 0).all()
    names = ("y", "gx", "gW1", "gb1", "gW2")
    for k, (name, got) in enumerate(zip(names, out)):
        got = got.double().cpu().numpy()
        w = want[k]
        if k == 0:
            assert not np.isnan(w).any()
        if c["dtype"] == BF16 and k < 2:
            gate_bf16(name, got, w)
        else:
            gate_f32(name, got, w, t32[k])
    return out


MASKS = {"none": dict(mask=None), "bool_ni": dict(mask="bool_ni"), "bool_1": dict(mask="bool_1")}
CASES = {
    # name: (shape, imputed channels, mask, hidden / NI, activation, extra)
    "odd_5x7_first": ((1, 2, 5, 7), [0], "none", 2, "gelu", {}),
    "odd_5x7_last": ((1, 2, 5, 7), [1], "bool_1", 2, "relu", {}),
    "odd_blocks_19x31": ((1, 3, 19, 31), [1], "bool_1", 2, "gelu", {}),
    "vec_8x16_unsorted": ((2, 7, 8, 16), [5, 0], "bool_ni", 2, "gelu", {}),
    "vec_8x16_last_xmask": ((2, 7, 8, 16), [6], "none", 2, "silu", dict(mask_channel=2)),
    "misaligned_8x16": ((2, 7, 8, 16), [5, 0], "bool_1", 2, "sin", dict(misaligned=True)),
    "leading_dims": ((2, 3, 7, 8, 16), [0], "none", 2, "gelu", {}),
    "blocks_91x180": ((1, 30, 91, 180), [5, 0], "none", 3, "gelu", dict(mask_channel=29)),
    "capacity_256_8_32": ((1, 256, 8, 16), [255, 3, 17, 0, 100, 64, 200, 31], "bool_ni", 4, "silu", {}),
}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mlp_imputation_against_fp64(name, dtype):
    shape, imp, mask, ratio, act, extra = CASES[name]
    print(f"\n{name} {dtype}")
    check_case(make_case(shape, imp, MASKS[mask]["mask"], dtype, ratio, **extra), act)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", ref.ACTS)
def test_the_four_activations(act, dtype):
    print(f"\n{act} {dtype}")
    check_case(make_case((2, 7, 8, 16), [5, 0], "bool_ni", dtype, 3, seed=7), act)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_no_pixel_masked_is_the_identity_with_zero_weight_gradients(dtype):
    c = make_case((2, 7, 8, 16), [5, 0], None, dtype, 2, masked="none")
    y, gx, gw1, gb1, gw2 = check_case(c, "gelu", expect="none")
    assert torch.equal(_bits(y), _bits(c["x"].to(DEV, dtype)))
    assert torch.equal(_bits(gx), _bits(c["g"].to(DEV, dtype)))
    for t in (gw1, gb1, gw2):
        assert (t == 0).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_every_pixel_masked(dtype):
    c = make_case((2, 7, 8, 16), [5, 0], None, dtype, 2, masked="all")
    _, gx, *_ = check_case(c, "gelu", expect="all")
    assert (gx[:, [5, 0]] == 0).all()


def test_a_float_mask_counts_any_nonzero_value():
    """a separate f32 mask with fractional values equals the bool mask of its nonzero entries"""
    c = make_case((2, 7, 8, 16), [5, 0], "bool_ni", F32, 2)
    mod = module_of(c, "gelu")
    want = run_module(mod, c)
    frac = torch.where(c["m"], torch.rand(c["m"].shape) * 0.5 + 0.01, torch.zeros(()))
    for m in (frac, frac.bfloat16()):
        got = run_module(mod, dict(c, m=m))
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_forward_and_backward_replay_from_a_captured_graph():
    c = make_case((2, 7, 8, 16), [5, 0], "bool_ni", F32, 2, seed=3)
    mod = module_of(c, "gelu")
    p = [mod.mlp.fwd[0].weight, mod.mlp.fwd[0].bias, mod.mlp.fwd[2].weight]
    x = c["x"].to(DEV).requires_grad_(True)
    g, m = c["g"].to(DEV), c["m"].to(DEV)

    def step():
        y = mod(x, m)
        return (y, *torch.autograd.grad(y, [x] + p, g))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [t.detach().clone() for t in eager]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        for t in out:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(_bits(a.detach()), _bits(b))


# ---- ConstantImputation ------------------------------------------------------------------------------------------------------
CONST_CASES = {
    "odd_5x7": ((1, 2, 5, 7), None),
    "vec_8x16_full_mask": ((2, 7, 8, 16), (2, 7, 8, 16)),
    "vec_8x16_one_plane": ((2, 7, 8, 16), (1, 1, 8, 16)),
    "leading_dims_per_channel": ((2, 3, 7, 8, 16), (7, 8, 16)),
    "chunks_91x180": ((1, 5, 91, 180), (1, 1, 91, 180)),
}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(CONST_CASES))
def test_constant_imputation_against_fp64(name, dtype):
    from makani_amd.imputation import ConstantImputation
    shape, mshape = CONST_CASES[name]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen).to(dtype).float()
    g = torch.randn(shape, generator=gen).to(dtype).float()
    x = torch.where(torch.rand(shape, generator=gen) < 0.2, torch.full((), float("nan")), x)
    m = None if mshape is None else torch.rand(mshape, generator=gen) < 0.3
    C = shape[-3]
    mod = ConstantImputation(C).to(DEV)
    w = mod.weight.detach().cpu().reshape(-1)
    flat = lambda t: t.reshape(-1, *shape[-3:])          # noqa: E731
    mfull = None if m is None else flat(m.expand(shape)).numpy()
    masked = torch.from_numpy(ref.const_mask(flat(x).numpy(), mfull))
    assert masked.any() and not masked.all()

    def run():
        xd = x.to(DEV, dtype).requires_grad_(True)
        y = mod(xd, None if m is None else m.to(DEV))
        return (y.detach(), *torch.autograd.grad(y, [xd, mod.weight], g.to(DEV, dtype)))

    y, gx, gw = run()
    for a, b in zip((y, gx, gw), run()):
        assert torch.equal(_bits(a), _bits(b))
    assert y.dtype == dtype and y.shape == x.shape and gw.shape == mod.weight.shape
    want_y = ref.const_fwd(flat(x).numpy(), mfull, w.numpy())
    want_gx, want_gw = ref.const_bwd(flat(x).numpy(), flat(g).numpy(), mfull)
    # the forward and the input gradient are selections: exact in either dtype (the fill value is rounded once)
    fill = w.to(dtype).double().view(1, -1, 1, 1).expand(masked.shape)
    assert torch.equal(flat(y).double().cpu(), torch.where(masked, fill, torch.from_numpy(want_y)))
    assert torch.equal(flat(gx).double().cpu(), torch.from_numpy(want_gx))
    xt = flat(x).to(DEV).requires_grad_(True)
    wt = w.to(DEV).requires_grad_(True)
    yt = ref.compose_const(xt, None if mfull is None else torch.from_numpy(mfull).to(DEV), wt)
    (gwt,) = torch.autograd.grad(yt, [wt], flat(g).to(DEV))
    print(f"\n{name} {dtype}")
    gate_f32("gw", gw.reshape(-1).double().cpu().numpy(), want_gw, gwt.double().cpu().numpy())


def test_cpu_tensors_raise():
    from makani_amd.imputation import ConstantImputation, MLPImputation
    with pytest.raises(RuntimeError, match="GPU"):
        MLPImputation(3, torch.tensor([1]))(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ConstantImputation(3)(torch.zeros(1, 3, 4, 4))
