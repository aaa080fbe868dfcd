"""``mk_fcn31_tail_fwd`` / ``mk_fcn31_tail_bwd`` on the GPU (``ops.Fcn31TailFn``) against the fp64 restatement of
tests/_impute_ref.py: y_c = clamp_c(d_c + [skip] xin[pred_ch[c]]), the gradient of d and, with the skip, the full input gradient
with zeros outside pred_ch.

The gates of tests/test_gpu_imputation.py.  f32: the kernel's largest error is at most 2 e_t + 4 2^-23 max|ref|, e_t the error of
the reference's composition in fp32 torch on the same inputs.  bf16: |y - ref| <= 2^-8 |ref| + 2^-23 max|ref| element by element.
Inputs are also placed exactly on the clamp's joints (v + off = 0 and 1/2)
and below 0, in numbers that are exact in bf16."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _impute_ref as ref          # noqa: E402
from test_gpu_imputation import _bits, _offset_view, gate_bf16, gate_f32          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

# name: (shape of d, Cin, water channels ("all" | list), skip, offsets, misaligned)
CASES = {
    "odd_5x7": ((1, 2, 5, 7), 4, [1], True, False, False),
    "odd_blocks_19x31": ((1, 3, 19, 31), 5, [0, 2], True, True, False),
    "vec_8x16": ((2, 7, 8, 16), 9, [5, 0], True, False, False),
    "vec_8x16_offsets": ((2, 7, 8, 16), 9, [6, 2, 3], True, True, False),
    "vec_8x16_no_skip": ((2, 7, 8, 16), 0, [1, 4], False, True, False),
    "misaligned_8x16": ((2, 7, 8, 16), 9, [5, 0], True, True, True),
    "leading_dims": ((2, 3, 7, 8, 16), 8, [0], True, False, False),
    "blocks_91x180": ((1, 30, 91, 180), 33, [3, 29, 11], True, True, False),
    "no_water": ((2, 7, 8, 16), 9, [], True, False, False),
    "all_water": ((2, 7, 8, 16), 7, "all", True, True, False),
    "all_water_no_skip": ((2, 7, 8, 16), 0, "all", False, False, False),
}


def make_case(name, dtype):
    shape, Cin, water, skip, offsets, misaligned = CASES[name]
    gen = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    *lead, Co, H, W = shape
    B = int(np.prod(lead)) if lead else 1
    water = list(range(Co)) if water == "all" else water
    d = (0.7 * torch.randn(B, Co, H, W, generator=gen)).to(dtype).float()
    g = torch.randn(B, Co, H, W, generator=gen).to(dtype).float()
    pred = torch.randperm(Cin, generator=gen)[:Co].tolist() if skip else None
    xin = (0.5 * torch.randn(B, Cin, H, W, generator=gen)).to(dtype).float() if skip else None
    # offsets exact in bf16, so that the joints below are exact in either dtype
    off = (torch.randint(-8, 9, (len(water),), generator=gen).float() / 16.0) if offsets and water else None
    if water:          # the joints and the flat part, at the first pixels of every water plane: v + off in {0, 1/2, -1/4, -3}
        o = torch.zeros(len(water)) if off is None else off
        for k, t in enumerate((0.0, 0.5, -0.25, -3.0)):
            v = (t - o).view(1, -1).expand(B, -1)
            if skip:
                xin[:, [pred[c] for c in water], 0, k] = 0.25
                v = v - 0.25
            d[:, water, 0, k] = v
    return dict(d=d, g=g, xin=xin, pred=pred, water=water, off=off, lead=lead, misaligned=misaligned, Cin=Cin)


def run_kernel(c, dtype):
    from makani_amd import ops
    Co = c["d"].shape[1]
    t = ops.tail_table(Co, c["water"], c["off"], c["pred"], c["Cin"], DEV)
    d = c["d"].to(DEV, dtype).view(*c["lead"], *c["d"].shape[1:])
    g = c["g"].to(DEV, dtype).view(d.shape)
    xin = None if c["xin"] is None else c["xin"].to(DEV, dtype).view(*c["lead"], *c["xin"].shape[1:])
    if c["misaligned"]:
        d, g = _offset_view(d), _offset_view(g)
    d.requires_grad_(True)
    ins = [d]
    if xin is not None:
        ins.append(xin.requires_grad_(True))
    y = ops.Fcn31TailFn.apply(d, xin, t)
    assert y.dtype == dtype and y.shape == d.shape
    grads = torch.autograd.grad(y, ins, g)
    B = c["d"].shape[0]
    return [y.detach().reshape(B, *d.shape[-3:])] + [t_.reshape(B, *t_.shape[-3:]) for t_ in grads]


def run_torch32(c):
    d = c["d"].to(DEV).requires_grad_(True)
    ins = [d]
    xin = None
    if c["xin"] is not None:
        xin = c["xin"].to(DEV).requires_grad_(True)
        ins.append(xin)
    y = ref.compose_tail(d, xin, c["pred"], c["water"], None if c["off"] is None else c["off"].to(DEV))
    grads = torch.autograd.grad(y, ins, c["g"].to(DEV))
    return [t.detach().double().cpu().numpy() for t in (y, *grads)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tail_against_fp64(name, dtype):
    c = make_case(name, dtype)
    out = run_kernel(c, dtype)
    for a, b in zip(out, run_kernel(c, dtype)):
        assert torch.equal(_bits(a), _bits(b)), "a second run differs"
    dn, gn = c["d"].numpy(), c["g"].numpy()
    xn = None if c["xin"] is None else c["xin"].numpy()
    off = None if c["off"] is None else c["off"].numpy()
    want = [ref.tail_fwd(dn, xn, c["pred"], c["water"], off), *ref.tail_bwd(dn, xn, gn, c["pred"], c["water"], off)]
    want = [w for w in want if w is not None]
    t32 = run_torch32(c)
    assert len(out) == len(want) == len(t32) == (3 if c["pred"] is not None else 2)
    print(f"\n{name} {dtype}")
    for nm, got, w, t in zip(("y", "gd", "gxin"), out, want, t32):
        assert torch.isfinite(got).all()
        if dtype == BF16:
            gate_bf16(nm, got.double().cpu().numpy(), w)
        else:
            gate_f32(nm, got.double().cpu().numpy(), w, t)
    if c["water"]:          # on the joints: y + off = 0, 1/4, 0, 0 and the slope 0, 1, 0, 0, exactly
        o = np.zeros(len(c["water"])) if off is None else off
        y, gd = out[0].double().cpu().numpy(), out[1].double().cpu().numpy()
        for k, (val, slope) in enumerate(((0.0, 0.0), (0.25, 1.0), (0.0, 0.0), (0.0, 0.0))):
            assert (y[:, c["water"], 0, k] == (val - o)[None]).all(), k
            assert (gd[:, c["water"], 0, k] == slope * gn[:, c["water"], 0, k]).all(), k
    if c["pred"] is not None:          # the input gradient: gd on pred_ch, exact zeros elsewhere
        gxin = out[2]
        rest = [ch for ch in range(c["Cin"]) if ch not in c["pred"]]
        assert torch.equal(_bits(gxin[:, c["pred"]]), _bits(out[1])) and (gxin[:, rest] == 0).all()
    if not c["water"] and c["pred"] is None:
        assert torch.equal(_bits(out[0]), _bits(c["d"].to(DEV, dtype)))


def test_mixed_dtypes_follow_the_decoder_output():
    """under autocast the decoder's output is bf16 and the network's input fp32: the reference adds ``residual.to(x.dtype)``, so the
    result and the traffic are bf16, and each gradient comes back in the dtype of its tensor"""
    from makani_amd import ops
    c = make_case("vec_8x16_offsets", BF16)
    t = ops.tail_table(c["d"].shape[1], c["water"], c["off"], c["pred"], c["Cin"], DEV)
    d = c["d"].to(DEV, BF16).requires_grad_(True)
    x32 = c["xin"].to(DEV).requires_grad_(True)          # (the values are exact in bf16)
    y = ops.Fcn31TailFn.apply(d, x32, t)
    gd, gx = torch.autograd.grad(y, [d, x32], c["g"].to(DEV, BF16))
    assert y.dtype == BF16 and gd.dtype == BF16 and gx.dtype == F32
    want = run_kernel(c, BF16)
    assert torch.equal(_bits(y), _bits(want[0])) and torch.equal(_bits(gd), _bits(want[1])) and torch.equal(gx, want[2].float())


def test_lists_are_checked_on_the_host():
    from makani_amd import ops
    with pytest.raises(ValueError, match="distinct"):
        ops.tail_table(4, [1, 1], None, None, 0, DEV)
    with pytest.raises(ValueError, match="distinct"):
        ops.tail_table(3, [0], None, [0, 1, 1], 5, DEV)
    with pytest.raises(ValueError, match="distinct"):
        ops.tail_table(3, [0], None, [0, 1, 7], 5, DEV)
