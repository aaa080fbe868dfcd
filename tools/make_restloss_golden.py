"""Record tests/golden/rest_losses.npz: the reference's own, unmodified SpectralAMSELoss (makani/utils/losses/amse_loss.py),
EnsembleNLLLoss (likelihood_loss.py) and GaussianMMDLoss (mmd_loss.py), imported through oracle.ref_shims and run in DOUBLE
precision, so that an fp64 restatement can be pinned against the record at rounding level.  Per case: int8-quantised inputs,
optional weights, the quadrature weights the class used, value, forecast (prediction) gradient and a JSON of class and kwargs.
Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_restloss_golden.py

Double precision without touching the classes: the modules are cast with ``.double()`` (the quadrature weights are the
class's fp32 values, widened: they are recorded); SpectralAMSELoss builds its transform with ``.float()`` and casts its inputs
``.to(torch.float32)``, so its transform gets the fp64 Legendre weights back after construction and ``torch.float32`` reads
as ``torch.float64`` while its forward runs (the inputs are int8 multiples of a power of two: exact either way).
GaussianMMDLoss(channel_reduction=True) is recorded with batch and channel axes exchanged (see the comment in main)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

NAMES = ["u500", "v500", "t2m"]
IMG = (17, 32)
# name, class, kwargs, E (0: deterministic), weights, NaN observations
CASES = [
    ("amse_default", "SpectralAMSELoss", dict(), 0, False, False),
    ("amse_weights", "SpectralAMSELoss", dict(), 0, True, False),
    ("nll_single_member_clamped", "EnsembleNLLLoss", dict(), 1, False, False),
    ("nll_three_members", "EnsembleNLLLoss", dict(), 3, False, False),
    ("nll_weights", "EnsembleNLLLoss", dict(), 2, True, False),
    ("mmd_default", "GaussianMMDLoss", dict(), 2, False, False),
    ("mmd_channel_reduction", "GaussianMMDLoss", dict(channel_reduction=True, sigma=16.0), 3, True, False),
    ("mmd_single_member", "GaussianMMDLoss", dict(), 1, False, False),
    ("mmd_alpha_beta1", "GaussianMMDLoss", dict(alpha=0.9, beta=1.0), 3, False, False),
    ("mmd_nan_observations", "GaussianMMDLoss", dict(sigma=2.0), 3, False, True),
]
MODULES = {"SpectralAMSELoss": "makani.utils.losses.amse_loss", "EnsembleNLLLoss": "makani.utils.losses.likelihood_loss",
           "GaussianMMDLoss": "makani.utils.losses.mmd_loss"}
SCALE = 1.0 / 32.0          # value = int8 * SCALE, exact in fp32; -128 stands for NaN


def main():
    from oracle import ref_shims
    from oracle import sht as osht
    ref_shims.install()
    # the ensemble classes scatter the spatial weights over the "ensemble" group even when it has one member; the serial shim
    # has no primitives: a split over a group of one is the identity
    maps = ref_shims.import_reference_module("makani.mpu.mappings")
    maps._split = lambda t, dim, group=None: t
    out = {}
    gen = torch.Generator().manual_seed(2026)
    B, C = 2, len(NAMES)
    for name, cls, extra, E, wgt, nan_obs in CASES:
        mod = ref_shims.import_reference_module(MODULES[cls])
        kwargs = dict(img_shape=list(IMG), crop_shape=list(IMG), crop_offset=[0, 0], channel_names=NAMES, grid_type="equiangular", **extra)
        loss = getattr(mod, cls)(**kwargs).double()
        lead = (B, E, C) if E else (B, C)
        aq = torch.clamp(torch.round(32.0 * torch.randn(*lead, *IMG, generator=gen)), -127, 127).to(torch.int8)
        bq = torch.clamp(torch.round(32.0 * torch.randn(B, C, *IMG, generator=gen)), -127, 127).to(torch.int8)
        if nan_obs:
            bq[torch.rand(bq.shape, generator=gen) < 0.05] = -128
        a = (aq.double() * SCALE).requires_grad_(True)
        b = torch.where(bq == -128, float("nan"), bq.double() * SCALE)
        w = None
        if cls == "SpectralAMSELoss":
            L = loss.sht.lmax
            loss.sht.weights = osht.RealSHT(*IMG, lmax=L, mmax=L, grid="equiangular").weights          # fp64 again
            w = (torch.rand(1, C, L, L, generator=gen) + 0.5).double() if wgt else None
            f32 = torch.float32
            torch.float32 = torch.float64
            try:
                val = loss(a, b, w)
            finally:
                torch.float32 = f32
        else:
            w = (torch.rand(B, C, *IMG, generator=gen) + 0.5).double() if wgt else None
            if extra.get("channel_reduction", False):
                # mmd_loss.py:192-194 sums `dim=-2` of the (E, B, C) / (E, E, B, C) distances: the BATCH axis, where its comment,
                # `n_channels` and the energy scores it is modelled on mean the channels.  The class is handed the inputs with
                # batch and channel axes exchanged, so that its own, unmodified arithmetic forms the channel sum: (1, B) -> (B, 1)
                val = loss(a.transpose(0, 2), b.transpose(0, 1), w.transpose(0, 1) if w is not None else None).transpose(0, 1)
                assert val.shape == (B, 1)
            else:
                val = loss(a, b, w)
            out[f"{name}/quad_weight"] = loss.quadrature.quad_weight.reshape(IMG).float().numpy()
        assert val.dtype == torch.float64, (name, val.dtype)
        (g,) = torch.autograd.grad(val.sum(), a)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(g).all()), name
        out[f"{name}/meta"] = np.array(json.dumps(dict(cls=cls, kwargs=kwargs, scale=SCALE)))
        out[f"{name}/a_i8"] = aq.numpy()
        out[f"{name}/b_i8"] = bq.numpy()
        if w is not None:
            out[f"{name}/weights"] = w.float().numpy()          # (drawn as fp32 values: the widening above is exact)
        out[f"{name}/out"] = val.detach().numpy()
        out[f"{name}/grad"] = g.numpy()
        print(name, tuple(val.shape), val.dtype, val.detach().reshape(-1)[:3].tolist())
    path = os.path.join(ROOT, "tests", "golden", "rest_losses.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
