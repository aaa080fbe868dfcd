"""Record tests/golden/vsht_losses.npz: the reference's own, unmodified GradientCRPSLoss / VortDivCRPSLoss
(makani/utils/losses/crps_loss.py), imported through oracle.ref_shims with the two vector transform classes of the test-side
fp64 restatement (tests/_vsht_ref.py) attached to the torch_harmonics shim at run time.  Needs the reference checkout
(MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_vsht_golden.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NAMES = ["u500", "v500", "u850", "v850", "t500"]
IMG = (17, 32)
CASES = [
    ("grad_skillspread_abs", "GradientCRPSLoss", dict(crps_type="skillspread", absolute=True), 3, True),
    ("grad_cdf_components", "GradientCRPSLoss", dict(crps_type="cdf", absolute=False), 4, False),
    ("grad_single_member_abs", "GradientCRPSLoss", dict(crps_type="skillspread", absolute=True), 1, False),
    ("grad_single_member_components", "GradientCRPSLoss", dict(crps_type="skillspread", absolute=False, lmax=12), 1, False),
    ("vortdiv_skillspread", "VortDivCRPSLoss", dict(crps_type="skillspread", alpha=0.95), 3, True),
    ("vortdiv_cdf", "VortDivCRPSLoss", dict(crps_type="cdf"), 2, False),
    ("vortdiv_single_member", "VortDivCRPSLoss", dict(crps_type="skillspread"), 1, False),
]


def main():
    from oracle import ref_shims
    import _vsht_ref as ref
    ref_shims.install()
    th = sys.modules["torch_harmonics"]

    class InverseF32(ref.InverseRealVectorSHT):
        """fp64 inside, fp32 out: the reference scatters the result back into its fp32 channels"""

        def forward(self, c):
            return super().forward(c).float()

    th.RealVectorSHT, th.InverseRealVectorSHT = ref.RealVectorSHT, InverseF32
    mod = ref_shims.import_reference_module("makani.utils.losses.crps_loss")
    # the two classes scatter the spatial weights over the "ensemble" group even when it has one member
    # (crps_loss.py:795,970); the serial shim has no primitives: a split over a group of one is the identity
    maps = ref_shims.import_reference_module("makani.mpu.mappings")
    maps._split = lambda t, dim, group=None: t
    out = {}
    gen = torch.Generator().manual_seed(2024)
    for name, cls, extra, E, wgt in CASES:
        kwargs = dict(img_shape=list(IMG), crop_shape=list(IMG), crop_offset=[0, 0], channel_names=NAMES, grid_type="equiangular", **extra)
        loss = getattr(mod, cls)(**kwargs)
        B, C = 2, len(NAMES)
        f = torch.randn(B, E, C, *IMG, generator=gen).requires_grad_(True)
        o = torch.randn(B, C, *IMG, generator=gen)
        w = torch.rand(B, C, *IMG, generator=gen) + 0.5 if wgt else None
        val = loss(f, o, w)
        (g,) = torch.autograd.grad(val.sum(), f)
        if cls == "GradientCRPSLoss" and extra.get("absolute"):
            with torch.no_grad():
                mag = loss.ivsht(torch.cat([loss.sht(f).unsqueeze(-3), torch.zeros_like(loss.sht(f)).unsqueeze(-3)], dim=-3)).pow(2).sum(-3).sqrt()
            print(f"{name}: smallest gradient magnitude {float(mag.min()):.3e} (median {float(mag.median()):.3e})")
        out[f"{name}/meta"] = np.array(json.dumps(dict(cls=cls, kwargs=kwargs)))
        out[f"{name}/forecasts"] = f.detach().numpy()
        out[f"{name}/observations"] = o.numpy()
        if w is not None:
            out[f"{name}/weights"] = w.numpy()
        out[f"{name}/out"] = val.detach().numpy()
        out[f"{name}/grad"] = g.numpy()
        print(name, tuple(val.shape), val.dtype, float(val.abs().mean()))
    path = os.path.join(ROOT, "tests", "golden", "vsht_losses.npz")
    np.savez(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
