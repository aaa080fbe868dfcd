"""The 384-row tile of the persistent ring kernel (csrc/conv1x1.hip: conv_nn_ring_kernel<6>, picked by conv_nn_ring_rows for
192 < M <= 384, K >= 512, plain or + bias, at least 256 pixel tiles).  It sums every output element in the order of the 192-row
tile, so its output is compared bit for bit with the same product run as two launches of at most 192 rows, which take that tile."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, M, K, H, W)
SHAPES = [
    (1, 384, 768, 256, 260),      # 260 tiles on 256 workgroups: four of them walk two tiles (aliased staging image, split prefetch)
    (1, 384, 768, 257, 264),      # 266 tiles, ragged last pixel tile: N % 256 = 8
    (2, 300, 768, 160, 208),      # batch (2 x 130 tiles) and rows past M
    (1, 384, 1344, 256, 258),     # 21 k-tiles
    (1, 384, 1354, 256, 258),     # ragged last k-tile: 10 of 64 channels
]
BELOW = (1, 384, 768, 16, 40)     # 3 pixel tiles: below the tile-count threshold, the plan keeps two 192-row tiles


def _dev():
    return torch.device("cuda:0")


def _operands(B, M, K, H, W):
    """as tests/test_gpu_kernels.py::test_conv1x1_nn_and_wgrad makes them"""
    torch.manual_seed(M + K)
    x = torch.randn(B, K, H, W).bfloat16()
    w = (torch.randn(M, K) / math.sqrt(K)).bfloat16()
    bias = torch.randn(M)
    return x.to(_dev()), w.to(_dev()), bias.to(_dev())


def _run(w, K, x, bias):
    from makani_amd import ops
    y, _ = ops.conv1x1_nn(ops.pad_weight_bf16(w), K, x, bias=bias)
    return y


@pytest.mark.parametrize("epi", ["plain", "bias"])
@pytest.mark.parametrize("B,M,K,H,W", SHAPES)
def test_384_row_tile_against_fp64_and_bit_for_bit_against_the_192_row_tile(B, M, K, H, W, epi):
    x, w, bias = _operands(B, M, K, H, W)
    if epi == "plain":
        bias = None
    y = _run(w, K, x, bias)
    ref = torch.einsum("mk,bkn->bmn", w.double(), x.double().view(B, K, H * W)).view(B, M, H, W)      # fp64, on the device
    if bias is not None:
        ref += bias.double().view(1, -1, 1, 1)
    err = rel_l2(y, ref.cpu())
    # the same product as a 192-row launch and the rest: the first runs the 192-row tile of the ring kernel; the second too for
    # M = 384 (192 rows), while the 108 rows left of M = 300 are fewer than the ring kernel takes and run the 128-row tile kernel
    # (conv_nn_plan), whose k-tiles are shorter: that part is held to the bf16 rounding gate, not to equality
    lo = _run(w[:192].contiguous(), K, x, None if bias is None else bias[:192].contiguous())
    hi = _run(w[192:].contiguous(), K, x, None if bias is None else bias[192:].contiguous())
    same_lo = torch.equal(y[:, :192], lo)
    ndiff_lo = int((y[:, :192] != lo).sum())
    if M - 192 >= 192:
        same_hi, hi_err = torch.equal(y[:, 192:], hi), 0.0
    else:
        same_hi, hi_err = True, rel_l2(y[:, 192:], hi.cpu().double())
    print(f"ring384 {(B, M, K, H, W)} {epi}: rel-L2 vs fp64 {err:.3e}; rows 0..191 differ in {ndiff_lo} elements; "
          f"rows 192.. equal {same_hi}, rel-L2 {hi_err:.3e}")
    assert err < 4e-3                                     # bf16 output rounding only (the gate of test_conv1x1_nn_and_wgrad)
    assert same_lo and same_hi
    assert hi_err < 4e-3


_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_gpu_conv_ring384 import _operands, _run
out = {{}}
for shape in {shapes!r}:
    x, w, bias = _operands(*shape)
    out[shape] = (_run(w, shape[2], x, None).cpu(), _run(w, shape[2], x, bias).cpu())
torch.save(out, {path!r})
"""


def _child(tmp_path, shapes, **env):
    path = str(tmp_path / "out.pt")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), shapes=shapes, path=path)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return torch.load(path)


def test_dispatch_boundary_and_the_override(tmp_path):
    """MAKANI_AMD_RING384=0 forces two 192-row tiles; the switch is read once per process, so that arm runs in a child process.
    Below the tile-count threshold this process takes the old tile by itself, above it the new one: both equal the forced result."""
    forced = _child(tmp_path, [BELOW, SHAPES[0]], MAKANI_AMD_RING384="0")
    for shape in (BELOW, SHAPES[0]):
        x, w, bias = _operands(*shape)
        assert torch.equal(_run(w, shape[2], x, None).cpu(), forced[shape][0]), shape
        assert torch.equal(_run(w, shape[2], x, bias).cpu(), forced[shape][1]), shape


def test_default_store_policy(tmp_path):
    """outputs of at most 256 MiB are stored with the streaming policy, so that is all the shapes above run; MAKANI_AMD_CONV_NT=0
    (read once per process) runs the 384-row tile with the default policy of the full-resolution launches: not a value may change"""
    plain_st = _child(tmp_path, [SHAPES[1]], MAKANI_AMD_CONV_NT="0")
    x, w, bias = _operands(*SHAPES[1])
    assert torch.equal(_run(w, SHAPES[1][2], x, None).cpu(), plain_st[SHAPES[1]][0])
    assert torch.equal(_run(w, SHAPES[1][2], x, bias).cpu(), plain_st[SHAPES[1]][1])
