"""The energy-score kernels (csrc/escore.hip) against the fp64 restatement of tests/_escore_ref.py at the smallest shapes that
reach every kernel path: a 91 x 180 grid (16 380 points: not a multiple of the block, several chunks), lmax = mmax = 46 (a
per-degree segment shorter than a wave), B = 2, C = 3; E = 2 (power of two), 5 (odd), 9 (two member tiles), 32 (the maximum);
p = 1, 2 (their own instantiations) and 2.5 (the exp2 / log2 path).  1e-5 on value and gradient (fp32); a
second pass on the same inputs is bit-identical.

The inputs.  The spectral forms go through the fp32 transform, which resolves a coefficient to about 2e-7 of the FIELD's
norm, while the gradient of a degree's norm is the unit vector along that degree's coefficient difference: a degree whose
differences are small against the field is resolved only to 2e-7 * |field| / |difference|, in any fp32 transform, whatever
the loss kernels do.  So the member part must carry comparable power at every degree and must not grow with E:
  * white noise (std 2) alone leaves the low degrees almost empty (per-degree sums of 1e-6 .. 1e-5 at l = 1, 2, i.e. at eps
    itself), so every member also gets a smooth large-scale part (2 x a 4 x 8 standard normal field, bilinearly interpolated);
  * its zonal mean is removed, so degree 0 (one coefficient, the area mean) is set by the member offsets 0.25 e alone:
    |difference| >= 0.25 less the noise of a plane mean (4 sigma = 0.1), the sum >= 0.15^2 / 4 pi = 1.8e-3;
  * the offsets stay below 8 for E = 32, the size of the common field (std 10).
In fp64 the smallest per-degree sum of these inputs is 4.8e-4, 2.8e-4, 1.7e-4, 3.3e-5 for E = 2, 5, 9, 32 (eps = 1e-6): no
degree is masked and none is near enough to eps for rounding to decide the mask (the mask itself: tests/test_escore.py)."""
import pytest
import torch
import torch.nn.functional as F

import _escore_ref as ref
from conftest import rel_l2

IMG, NAMES = (91, 180), ["u500", "v500", "t2m"]
FORMS = [("LpEnergyScoreLoss", dict(p=1.0)), ("LpEnergyScoreLoss", dict(p=2.0, channel_reduction=False)),
         ("LpEnergyScoreLoss", dict(p=2.5, beta=0.9)), ("SobolevEnergyScoreLoss", dict(lmax=46, grid_type="legendre-gauss")),
         ("SpectralL2EnergyScoreLoss", dict(lmax=46, grid_type="legendre-gauss", channel_reduction=False, alpha=0.95))]


@pytest.mark.gpu
@pytest.mark.parametrize("E", [2, 5, 9, 32])
@pytest.mark.parametrize("form", range(len(FORMS)))
def test_escore_matches_fp64_restatement_and_is_deterministic(form, E):
    import makani_amd as ma
    cls, extra = FORMS[form]
    kwargs = dict(dict(img_shape=IMG, crop_shape=IMG, crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular"), **extra)
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(100 * form + E)
    B, C = 2, len(NAMES)
    # members of a trained ensemble are close: a common field plus a small member part (the spread lives in the low digits);
    # the member part is white noise + a smooth zonal-mean-free field + a distinct mean (see the module docstring)
    o = (10.0 * torch.randn(B, C, *IMG, generator=gen)).to(dev)
    smooth = F.interpolate(torch.randn(B * E * C, 1, 4, 8, generator=gen), size=IMG, mode="bilinear", align_corners=True)
    smooth = (smooth - smooth.mean(-1, keepdim=True)).reshape(B, E, C, *IMG)
    f = (o.cpu().unsqueeze(1) + 2.0 * torch.randn(B, E, C, *IMG, generator=gen) + 2.0 * smooth
         + 0.25 * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)).to(dev)
    w = (torch.rand(B, C, *IMG, generator=gen) + 0.5).to(dev) if cls == "LpEnergyScoreLoss" else None
    g_out = torch.randn(B, 1 if kwargs.get("channel_reduction", True) else C, generator=gen).to(dev)
    mod = getattr(ma, cls)(**kwargs).to(dev)
    if cls != "LpEnergyScoreLoss":
        assert mod.sht.lmax == 46 and mod.sht.mmax == 46
    runs = []
    for _ in range(2):
        fx = f.clone().requires_grad_(True)
        out = mod(fx, o, w) if w is not None else mod(fx, o)
        (g,) = torch.autograd.grad((out * g_out).sum(), fx)
        runs.append((out, g))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    fr = f.double().requires_grad_(True)
    want = ref.reference(cls, kwargs, fr, o, w)
    (gw,) = torch.autograd.grad((want * g_out.double()).sum(), fr)
    out, g = runs[0]
    print(f"{cls} {extra} E={E}: value {rel_l2(out, want):.2e} gradient {rel_l2(g, gw):.2e}")
    assert out.shape == want.shape
    assert rel_l2(out, want) < 1e-5, rel_l2(out, want)
    assert rel_l2(g, gw) < 1e-5, rel_l2(g, gw)
