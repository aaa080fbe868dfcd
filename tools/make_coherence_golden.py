"""Record tests/golden/coherence_losses.npz: the reference's own, unmodified SpectralCoherenceLoss
(makani/utils/losses/energy_score.py), CoherenceRegularization and SpectralRegularization (regularization.py), imported through
oracle.ref_shims and run in DOUBLE precision, so that the fp64 restatement of tests/_coherence_ref.py can be pinned against the
record at rounding level.  Per case: int8-quantised inputs (plus a mean per field), value, forecast gradient and a JSON of class and kwargs.  Needs the
reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_coherence_golden.py

Double precision without touching the classes: the modules are cast with ``.double()`` (their weights are 0, 1 and 2: exact),
the transform gets the fp64 Legendre weights back after construction (the classes build it with ``.float()``), and
``Tensor.float()`` — the classes' ``self.sht(forecasts.float())`` — hands back the fp64 tensor while a forward runs (the inputs
are int8 multiples of a power of two: exact either way)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

NAMES = ["u500", "v500", "t2m"]
IMG = (17, 32)
# name, class, kwargs, E (0: forecasts without a member axis)
CASES = [
    ("coherence_default", "SpectralCoherenceLoss", dict(), 3),
    ("coherence_relative_per_channel", "SpectralCoherenceLoss", dict(relative=True, channel_reduction=False), 4),
    ("coherence_single_member", "SpectralCoherenceLoss", dict(), 1),
    ("coherence_lmax", "SpectralCoherenceLoss", dict(lmax=12), 3),
    ("cohreg_band_inter", "CoherenceRegularization", dict(lmin=3, lmax=12, ensemble_coherence_weight=0.5), 3),
    ("cohreg_default_single_member", "CoherenceRegularization", dict(), 1),
    ("cohreg_default", "CoherenceRegularization", dict(), 3),
    ("specreg_default", "SpectralRegularization", dict(), 3),
    ("specreg_logarithmic", "SpectralRegularization", dict(logarithmic=True), 2),
    ("specreg_four_dimensional", "SpectralRegularization", dict(), 0),
]
MODULES = {"SpectralCoherenceLoss": "makani.utils.losses.energy_score", "CoherenceRegularization": "makani.utils.losses.regularization",
           "SpectralRegularization": "makani.utils.losses.regularization"}
SCALE = 1.0 / 32.0          # value = int8 * SCALE + mean, exact in fp32
# every field gets a mean of its own: the mean is the ONE coefficient of degree 0, and without it that degree's power is a small
# random number which the relative form divides by.  Member e: A_MEAN + A_STEP * e; observation: B_MEAN
A_MEAN, A_STEP, B_MEAN = 0.5, 0.125, 1.0


def main():
    from oracle import ref_shims
    from oracle import sht as osht
    ref_shims.install()
    out = {}
    gen = torch.Generator().manual_seed(2027)
    B, C = 2, len(NAMES)
    for name, cls, extra, E in CASES:
        mod = ref_shims.import_reference_module(MODULES[cls])
        kwargs = dict(img_shape=list(IMG), crop_shape=list(IMG), crop_offset=[0, 0], channel_names=NAMES, grid_type="equiangular", **extra)
        loss = getattr(mod, cls)(**kwargs).double()
        L = loss.sht.lmax
        loss.sht.weights = osht.RealSHT(*IMG, lmax=L, mmax=L, grid="equiangular").weights          # fp64 again
        lead = (B, E, C) if E else (B, C)
        aq = torch.clamp(torch.round(32.0 * torch.randn(*lead, *IMG, generator=gen)), -127, 127).to(torch.int8)
        bq = torch.clamp(torch.round(32.0 * torch.randn(B, C, *IMG, generator=gen)), -127, 127).to(torch.int8)
        means = (A_MEAN + A_STEP * torch.arange(E, dtype=torch.float64)).reshape(1, E, 1, 1, 1) if E else A_MEAN
        a = (aq.double() * SCALE + means).requires_grad_(True)
        b = bq.double() * SCALE + B_MEAN
        to_float = torch.Tensor.float
        torch.Tensor.float = lambda t: t.double()
        try:
            val = loss(a, b)
        finally:
            torch.Tensor.float = to_float
        assert val.dtype == torch.float64, (name, val.dtype)
        (g,) = torch.autograd.grad(val.sum(), a)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(g).all()), name
        out[f"{name}/meta"] = np.array(json.dumps(dict(cls=cls, kwargs=kwargs, scale=SCALE, a_mean=A_MEAN, a_step=A_STEP, b_mean=B_MEAN)))
        out[f"{name}/a_i8"] = aq.numpy()
        out[f"{name}/b_i8"] = bq.numpy()
        out[f"{name}/out"] = val.detach().numpy()
        out[f"{name}/grad"] = g.numpy()
        print(name, tuple(val.shape), val.dtype, val.detach().reshape(-1)[:3].tolist())
    path = os.path.join(ROOT, "tests", "golden", "coherence_losses.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
