"""Record tests/golden/escorr_losses.npz: the reference's own, unmodified CorrectedSpectralL2EnergyScoreLoss
(makani/utils/losses/energy_score.py:859-1042), imported through oracle.ref_shims.  Per case: int8-coded inputs, value, forecast
gradient and a JSON of class and kwargs, in the layout of tools/make_escore_golden.py (tests/_escore_ref.load_cases reads both).
Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_escorr_golden.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

NAMES = ["u500", "v500", "t2m"]
IMG = (17, 32)
CLS = "CorrectedSpectralL2EnergyScoreLoss"
# name, kwargs, E, amplitude of the observation relative to the members'
CASES = [
    ("corrected_default", dict(), 3, 1.0),
    ("corrected_per_channel_lmax", dict(channel_reduction=False, lmax=12, alpha=0.9, beta=0.8), 4, 1.0),
    ("corrected_single_member", dict(), 1, 1.0),
    ("corrected_ratio_far_from_one", dict(), 2, 1.0 / 3.0),          # members of 3 x the observation's amplitude
]


def main():
    from oracle import ref_shims
    ref_shims.install()
    mod = ref_shims.import_reference_module("makani.utils.losses.energy_score")
    out = {}
    gen = torch.Generator().manual_seed(2026)
    eps = 1.0e-6
    for name, extra, E, obs_amp in CASES:
        kwargs = dict(img_shape=list(IMG), crop_shape=list(IMG), crop_offset=[0, 0], channel_names=NAMES, grid_type="equiangular", **extra)
        loss = getattr(mod, CLS)(**kwargs)
        loss.train(False)
        B, C = 2, len(NAMES)
        # value = int8 * scale + member_offset * (e + 1), exact in fp32; fields of amplitude 10 with distinct means keep every
        # degree's sum (a few coefficients of one channel) well above eps
        amp = 10.0
        scale, member_offset = amp / 32.0, amp - 1.0
        fq = torch.clamp(torch.round(32.0 * torch.randn(B, E, C, *IMG, generator=gen)), -127, 127).to(torch.int8)
        oq = torch.clamp(torch.round(32.0 * obs_amp * torch.randn(B, C, *IMG, generator=gen)), -127, 127).to(torch.int8)
        f = fq.float() * scale + member_offset * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
        f.requires_grad_(True)
        o = oq.float() * scale
        # the smallest (channel-reduced) sum the eps mask sees: recorded by watching torch.where's mask operands
        seen = []
        real_where = torch.where

        def where(cond, a, b=None, *rest):
            if b is not None and isinstance(b, torch.Tensor) and isinstance(a, float) and a == eps:
                seen.append(b.detach())
            return real_where(cond, a, b, *rest)

        mod.torch.where = where
        try:
            val = loss(f, o)
        finally:
            mod.torch.where = real_where
        (g,) = torch.autograd.grad(val.sum(), f)
        sums = torch.cat([s.reshape(-1) for s in seen])
        sums = sums[sums > 0]                          # the (e, e) diagonal is exactly 0: masked either way
        assert not bool(((sums < 100 * eps) & (sums > eps / 100)).any()), f"{name}: a sum within a factor 100 of eps"
        print(f"{name}: smallest non-zero channel-reduced sum {float(sums.min()):.3e}")
        out[f"{name}/meta"] = np.array(json.dumps(dict(cls=CLS, kwargs=kwargs, train=False, scale=scale, member_offset=member_offset)))
        out[f"{name}/forecasts_i8"] = fq.numpy()
        out[f"{name}/observations_i8"] = oq.numpy()
        out[f"{name}/out"] = val.detach().numpy()
        out[f"{name}/grad"] = g.numpy()
        print(name, tuple(val.shape), val.dtype, float(val.detach().abs().mean()))
    path = os.path.join(ROOT, "tests", "golden", "escorr_losses.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
