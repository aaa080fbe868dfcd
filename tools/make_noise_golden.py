"""Record tests/golden/noise.npz: the reference's own, unmodified noise processes (makani/models/noise.py), imported through
oracle.ref_shims and run on the CPU over the oracle's inverse SHT.  Per case: a JSON of class, constructor kwargs and the
sequence of updates; sigma_l / phi / discount; per update the innovations xi (drawn from a clone of the module's CPU generator
taken just before the update) and the state after it; the field forward() of the last state; for the learnable isotropic case
the sigma_l gradient of sum(field * g) for a recorded g.  Every update is cross-checked here against the fp64 restatement
in tests/_noise_ref.py driven by the recorded xi.  Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the
repository root:  python tools/make_noise_golden.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

B = 2
# name, class, kwargs (batch_size is B), updates (replace_state flags)
CASES = [
    ("diffusion_per_channel_lists", "DiffusionNoiseS2",
     dict(img_shape=[9, 16], num_channels=3, num_time_steps=1, sigma=1.5, kT=[0.05, 0.01, 0.002], lambd=[1.0, 0.5, 2.0]), [True, False]),
    ("diffusion_history_legendre_gauss", "DiffusionNoiseS2",
     dict(img_shape=[9, 16], num_channels=2, num_time_steps=3, grid_type="legendre-gauss", lmax=6, kT=0.02, lambd=0.7, seed=7),
     [True, False, False]),
    ("diffusion_reflect", "DiffusionNoiseS2",
     dict(img_shape=[9, 16], num_channels=1, num_time_steps=1, reflect=True, kT=0.01), [True, False]),
    ("isotropic_alpha", "IsotropicGaussianRandomFieldS2",
     dict(img_shape=[9, 16], num_channels=2, num_time_steps=1, sigma=2.0, alpha=1.5), [False]),
    ("isotropic_learnable", "IsotropicGaussianRandomFieldS2",
     dict(img_shape=[17, 32], num_channels=1, num_time_steps=1, alpha=0.5, learnable=True, seed=11), [False]),
    ("dummy_constant_random", "DummyNoiseS2",
     dict(img_shape=[9, 16], num_channels=1, num_time_steps=2, mode="constant_random"), [False]),
]


def main():
    from oracle import ref_shims
    import _noise_ref as R
    mod = ref_shims.import_reference_module("makani.models.noise")
    out = {}
    for name, cls, kwargs, updates in CASES:
        m = getattr(mod, cls)(batch_size=B, **kwargs)
        out[f"{name}/meta"] = np.array(json.dumps(dict(cls=cls, kwargs=kwargs, batch_size=B, updates=updates)))
        for buf in ("sigma_l", "phi", "discount"):
            if hasattr(m, buf):
                out[f"{name}/{buf}"] = getattr(m, buf).detach().numpy().copy()
        out[f"{name}/state_init"] = m.state.numpy().copy()
        diffusion = cls == "DiffusionNoiseS2"
        for k, replace in enumerate(updates):
            before = m.state.numpy().astype(np.float64)
            clone = torch.Generator(device="cpu")
            clone.set_state(m.rng_cpu.get_state())
            shape = list(m.state.shape)
            if diffusion and not replace:
                shape[1] = 1
            xi = torch.empty(shape, dtype=torch.float32).normal_(mean=0.0, std=1.0, generator=clone)
            m.update(replace_state=replace)
            after = m.state.numpy().copy()
            # the clone drew what the module drew: the restated update rule over xi gives the module's new state
            if diffusion:
                want = R.update(before, xi.numpy().astype(np.float64), "replace" if replace else "ar",
                                m.sigma_l.detach().numpy().astype(np.float64).reshape(m.num_channels, m.lmax),
                                m.phi.detach().numpy().astype(np.float64).reshape(-1), m.reflect)
            else:
                want = R.update(before, xi.numpy().astype(np.float64), "white", reflect=m.reflect)
            err = R.rel_l2(after, want)
            assert err < 1e-6, (name, k, err)
            out[f"{name}/xi_{k}"] = xi.numpy()
            out[f"{name}/state_{k}"] = after
        field = m()
        out[f"{name}/field"] = field.detach().numpy().copy()
        if kwargs.get("learnable", False) and not diffusion:
            g = torch.randn(field.shape, generator=torch.Generator().manual_seed(5))
            (grad,) = torch.autograd.grad((field * g).sum(), m.sigma_l)
            out[f"{name}/g"] = g.numpy()
            out[f"{name}/sigma_l_grad"] = grad.numpy()
        print(name, tuple(m.state.shape), "field", tuple(field.shape), float(field.detach().abs().mean()))
    path = os.path.join(ROOT, "tests", "golden", "noise.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
