"""Record tests/golden/escore_losses.npz: the reference's own, unmodified LpEnergyScoreLoss / SobolevEnergyScoreLoss /
SpectralL2EnergyScoreLoss (makani/utils/losses/energy_score.py), imported through oracle.ref_shims.  Per case: inputs, optional
spatial weights / lead_time_step, value, forecast gradient and a JSON of class and kwargs.  Needs the reference checkout
(MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_escore_golden.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

NAMES = ["u500", "v500", "t850", "z500", "t2m"]
IMG = (17, 32)
# name, class, kwargs, E, spatial weights, NaN observations, (train mode, lead_time_step)
CASES = [
    ("lp_p2_weights", "LpEnergyScoreLoss", dict(p=2.0), 3, True, False, None),
    ("lp_p1.5_beta_per_channel", "LpEnergyScoreLoss", dict(p=1.5, beta=0.8, channel_reduction=False), 4, False, False, None),
    ("lp_p1_alpha", "LpEnergyScoreLoss", dict(p=1.0, alpha=0.9), 2, False, False, None),
    ("lp_single_member", "LpEnergyScoreLoss", dict(), 1, False, False, None),
    ("lp_nan_observations", "LpEnergyScoreLoss", dict(), 3, False, True, None),
    ("lp_spread_temper", "LpEnergyScoreLoss", dict(spread_temper_steps=4, channel_reduction=False), 3, False, False, [1.0, 2.0, 6.0, 8.0, 3.0]),
    ("sobolev_default", "SobolevEnergyScoreLoss", dict(), 3, False, False, None),
    ("sobolev_params_per_channel", "SobolevEnergyScoreLoss",
     dict(fraction=0.5, offset=0.5, relative_weight=2.0, alpha=0.9, channel_reduction=False), 4, False, False, None),
    ("spectral_default", "SpectralL2EnergyScoreLoss", dict(), 3, False, False, None),
    ("spectral_per_channel_lmax", "SpectralL2EnergyScoreLoss", dict(channel_reduction=False, lmax=12), 2, False, False, None),
    ("spectral_single_member", "SpectralL2EnergyScoreLoss", dict(), 1, False, False, None),
]


def main():
    from oracle import ref_shims
    ref_shims.install()
    mod = ref_shims.import_reference_module("makani.utils.losses.energy_score")
    # LpEnergyScoreLoss scatters the spatial weights over the "ensemble" group even when it has one member; the serial shim
    # has no primitives: a split over a group of one is the identity
    maps = ref_shims.import_reference_module("makani.mpu.mappings")
    maps._split = lambda t, dim, group=None: t
    out = {}
    gen = torch.Generator().manual_seed(2025)
    eps = 1.0e-6
    for name, cls, extra, E, wgt, nan_obs, temper in CASES:
        kwargs = dict(img_shape=list(IMG), crop_shape=list(IMG), crop_offset=[0, 0], channel_names=NAMES, grid_type="equiangular", **extra)
        loss = getattr(mod, cls)(**kwargs)
        loss.train(temper is not None)
        B, C = 2, len(NAMES)
        # inputs are stored as int8 (the file has to stay small): value = int8 * scale + member_offset * (e + 1), exact in fp32;
        # -128 stands for NaN.  The per-degree score masks every degree on its own: fields of amplitude 10 with distinct
        # means keep each degree's sum (a few coefficients of one channel) well above eps
        amp = 10.0 if cls == "SpectralL2EnergyScoreLoss" else 1.0
        scale, member_offset = amp / 32.0, amp - 1.0
        fq = torch.clamp(torch.round(32.0 * torch.randn(B, E, C, *IMG, generator=gen)), -127, 127).to(torch.int8)
        oq = torch.clamp(torch.round(32.0 * torch.randn(B, C, *IMG, generator=gen)), -127, 127).to(torch.int8)
        if nan_obs:
            oq[torch.rand(oq.shape, generator=gen) < 0.05] = -128
        f = fq.float() * scale + member_offset * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
        f.requires_grad_(True)
        o = torch.where(oq == -128, float("nan"), oq.float() * scale)
        w = torch.rand(B, C, *IMG, generator=gen) + 0.5 if wgt else None
        lts = torch.tensor(temper) if temper is not None else None
        # the smallest (channel-reduced) sum the eps mask sees: recorded by watching torch.where's mask operands
        seen = []
        real_where = torch.where

        def where(cond, a, b=None, *rest):
            if b is not None and isinstance(b, torch.Tensor) and isinstance(a, float) and a == eps:
                seen.append(b.detach())
            return real_where(cond, a, b, *rest)

        mod.torch.where = where
        try:
            if cls == "LpEnergyScoreLoss":
                val = loss(f, o, w, lead_time_step=lts)
            else:
                val = loss(f, o)
        finally:
            mod.torch.where = real_where
        (g,) = torch.autograd.grad(val.sum(), f)
        sums = torch.cat([s.reshape(-1) for s in seen])
        sums = sums[sums > 0]                          # the spectral classes' (e, e) diagonal is exactly 0: masked either way
        lo = float(sums.min())
        assert not bool(((sums < 100 * eps) & (sums > eps / 100)).any()), f"{name}: a sum within a factor 100 of eps"
        print(f"{name}: smallest non-zero channel-reduced sum {lo:.3e}")
        out[f"{name}/meta"] = np.array(json.dumps(dict(cls=cls, kwargs=kwargs, train=temper is not None, scale=scale,
                                                          member_offset=member_offset)))
        out[f"{name}/forecasts_i8"] = fq.numpy()
        out[f"{name}/observations_i8"] = oq.numpy()
        if w is not None:
            out[f"{name}/weights"] = w.numpy()
        if lts is not None:
            out[f"{name}/lead_time_step"] = lts.numpy()
        out[f"{name}/out"] = val.detach().numpy()
        out[f"{name}/grad"] = g.numpy()
        print(name, tuple(val.shape), val.dtype, float(val.abs().mean()))
    path = os.path.join(ROOT, "tests", "golden", "escore_losses.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
