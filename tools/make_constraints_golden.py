"""Record tests/golden/constraints.npz: the reference's own, unmodified ``_HydrostaticBalanceWrapper``
(makani/models/parametrizations.py), ``HydrostaticBalanceProjection`` and ``NonNegativeConstraint`` (makani/utils/constraints.py),
imported through oracle.ref_shims.  Per case: channel names and constructor kwargs (JSON), bias and scale, every buffer the class
built, the input and the upstream gradient, output and input gradient of a DOUBLE-precision run, and ``err32_out`` /
``err32_grad``: the max-abs difference between the class's own fp32 CPU run and that double run (what the GPU tests gate on).
Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_constraints_golden.py

Double precision without touching the classes: the module is cast with ``.double()`` (its buffers are the class's fp32 values,
widened: they are recorded as built) and, while ``forward`` runs, ``torch.float32`` reads as ``torch.float64`` and
``Tensor.float`` as ``Tensor.double`` (the classes force fp32 with exactly these two).  The inputs and upstream gradients are
multiples of 1/32 with |n| <= 127: exact in bf16, fp32 and fp64."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

B, H, W = 2, 5, 7
SURFACE = {"u10m": (0.5, 5.0), "v10m": (-0.2, 4.0), "t2m": (278.0, 21.0), "sp": (9.7e4, 9.0e3), "tcwv": (18.0, 16.0)}


def stats_of(names):
    """normalisation statistics of realistic size per channel name: (1, C, 1, 1) bias and scale, fp32"""
    bias, scale = [], []
    for n in names:
        if n in SURFACE:
            b, s = SURFACE[n]
        else:
            p = int(n[1:])
            k = math.log(1000.0 / p) / math.log(20.0)          # 0 at 1000 hPa, 1 at 50 hPa
            b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3 * (0.8 + 0.4 * k)), "t": (285.0 - 70.0 * k, 15.0 - 6.0 * k),
                    "q": (2.0e-3 * (1.0 - k) ** 3 + 2e-6, 2.0e-3 * (1.0 - k) ** 3 + 1e-6), "u": (3.0 + 10.0 * k, 8.0 + 6.0 * k)}[n[0]]
        bias.append(b)
        scale.append(s)
    return (torch.tensor(bias, dtype=torch.float32).view(1, -1, 1, 1), torch.tensor(scale, dtype=torch.float32).view(1, -1, 1, 1))


# t / z / q interleaved with surface channels, not in pressure order
SMALL = ["u10m", "t500", "z850", "q500", "t2m", "z250", "t850", "q250", "z500", "sp", "q850", "t250"]
TWO = ["z500", "u10m", "t850", "q850", "t500", "z850", "q500"]
LEVELS13 = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
WIDE = ["u10m"] + [f"{v}{p}" for p in (500, 50, 925, 250, 1000, 100, 700, 300, 150, 850, 400, 200, 600) for v in ("z", "t")] + ["sp", "tcwv"]
NN = ["u10m", "q500", "tcwv", "t2m", "q850"]

# name, kind, channel names, constructor kwargs (bias / scale / climatology_offset are filled in below), with statistics, training
CASES = [
    ("wrapper_dry", "wrapper", SMALL, dict(p_min=50, p_max=900, use_moist_air_formula=False), True, True),
    ("wrapper_moist", "wrapper", SMALL, dict(p_min=50, p_max=900, use_moist_air_formula=True), True, True),
    ("wrapper_two_levels", "wrapper", TWO, dict(p_min=50, p_max=900, use_moist_air_formula=True), True, True),
    ("wrapper_window_of_13", "wrapper", WIDE, dict(p_min=100, p_max=900, use_moist_air_formula=False), True, True),
    ("wrapper_no_stats", "wrapper", SMALL, dict(p_min=50, p_max=900, use_moist_air_formula=False), False, True),
]
for moist in (False, True):
    for strength in (1.0, 0.7):
        for clim in (False, True):
            CASES.append((f"projection_{'moist' if moist else 'dry'}_s{int(strength * 10):02d}{'_clim' if clim else ''}", "projection", SMALL,
                          dict(p_min=50, p_max=900, strength=strength, use_moist_air_formula=moist, climatology_offset=clim), True, True))
CASES += [
    ("projection_window_of_13", "projection", WIDE, dict(p_min=100, p_max=900, strength=1.0, use_moist_air_formula=False, climatology_offset=True), True, True),
    ("projection_two_levels", "projection", TWO, dict(p_min=50, p_max=900, strength=0.7, use_moist_air_formula=True, climatology_offset=None), True, True),
]
for mode, training in (("silu", True), ("softplus", True), ("silu", False)):
    for with_stats in (True, False):
        CASES.append((f"nonneg_{mode if training else 'eval'}{'' if with_stats else '_no_stats'}", "nonneg", NN,
                      dict(names_to_clamp=["q500", "q850", "tcwv", "not_there"], eps=0.1, mode=mode, leak=0.02), with_stats, training))


def quantised(shape, gen):
    return torch.clamp(torch.round(32.0 * torch.randn(*shape, generator=gen)), -127, 127) / 32.0


def run(module, x, g, double):
    """output and input gradient of the class's own forward, in fp32 or (see the module docstring) in fp64"""
    f32, tfloat = torch.float32, torch.Tensor.float
    x = (x.double() if double else x.float()).clone().requires_grad_(True)
    if double:
        module = module.double()
        torch.float32, torch.Tensor.float = torch.float64, torch.Tensor.double
    try:
        out = module(x)
    finally:
        torch.float32, torch.Tensor.float = f32, tfloat
    assert out.dtype == (torch.float64 if double else torch.float32), out.dtype
    (gx,) = torch.autograd.grad(out, x, g.to(out.dtype))
    return out.detach(), gx


def main():
    from oracle import ref_shims
    ref_shims.install()
    par = ref_shims.import_reference_module("makani.models.parametrizations")
    con = ref_shims.import_reference_module("makani.utils.constraints")
    gen = torch.Generator().manual_seed(2027)
    out = {}
    for name, kind, names, kwargs, with_stats, training in CASES:
        bias, scale = stats_of(names) if with_stats else (None, None)
        kw = dict(kwargs)
        meta = dict(kind=kind, channel_names=names, kwargs=dict(kwargs), with_stats=with_stats, training=training)
        if kind == "projection" and kw["climatology_offset"]:
            n_all = len(con.get_matching_channels_pl(names, "z", "t", float("-inf"), float("inf"))[2])
            kw["climatology_offset"] = 40.0 * torch.randn(n_all - 1, generator=gen).float()
            out[f"{name}/climatology_offset"] = kw["climatology_offset"].numpy()
        elif kind == "projection":
            kw["climatology_offset"] = None
        if kind == "projection":          # (the JSON says whether the case has one; the values are the array above)
            meta["kwargs"]["climatology_offset"] = kw["climatology_offset"] is not None

        def make():
            cls = {"wrapper": par._HydrostaticBalanceWrapper, "projection": con.HydrostaticBalanceProjection,
                   "nonneg": con.NonNegativeConstraint}[kind]
            m = cls(channel_names=names, bias=bias, scale=scale, **kw)
            return m.train(training)

        mod = make()
        c_in = mod.mapping.shape[1] if kind == "wrapper" else len(names)
        x = quantised((B, c_in, H, W), gen)
        if kind == "nonneg" and not training:          # no result may depend on a tie: keep 1e-3 and more off the clamp point
            lo = torch.zeros(1, c_in, 1, 1)
            if mod.offset is not None:
                lo[:, mod.channel_indices] = -mod.offset
            near = (x - lo).abs() < 1e-3
            x = torch.where(near, x + 1.0 / 32.0, x)
            assert not bool(((x - lo).abs() < 1e-3).any())
        g = quantised((B, len(names), H, W), gen)
        for bname, buf in mod.named_buffers():
            out[f"{name}/buf/{bname}"] = buf.detach().clone().numpy()
        meta["persistent"] = sorted(mod.state_dict().keys())
        if kind == "wrapper":
            meta.update(z_idx=mod.z_idx, t_idx=mod.t_idx, aux_idx=mod.aux_idx, pressures=mod.pressures, moist=bool(mod.use_moist_air_formula),
                        N_in_channels=int(mod.mapping.shape[1]))
            if mod.use_moist_air_formula:
                meta["q_idx"] = mod.q_idx
        elif kind == "projection":
            meta.update(channel_indices=mod.channel_indices.tolist(), num_levels=mod.num_levels, strength=mod.strength,
                        moist=bool(mod.use_moist_air_formula))
            if mod.use_moist_air_formula:
                meta["q_indices"] = mod.q_indices.tolist()
        else:
            meta.update(channel_indices=mod.channel_indices.tolist(), eps=mod.eps, leak=mod.leak, mode=mod.mode)
        o32, g32 = run(make(), x, g, False)
        o64, g64 = run(make(), x, g, True)
        assert bool(torch.isfinite(o64).all()) and bool(torch.isfinite(g64).all()), name
        e_out, e_grad = (o32.double() - o64).abs().max().item(), (g32.double() - g64).abs().max().item()
        if bias is not None:
            out[f"{name}/bias"], out[f"{name}/scale"] = bias.numpy(), scale.numpy()
        out[f"{name}/meta"] = np.array(json.dumps(meta))
        out[f"{name}/x"] = x.float().numpy()
        out[f"{name}/g"] = g.float().numpy()
        out[f"{name}/out"] = o64.numpy()
        out[f"{name}/grad"] = g64.numpy()
        out[f"{name}/err32_out"] = np.array(e_out)
        out[f"{name}/err32_grad"] = np.array(e_grad)
        print(f"{name:34s} C {c_in:3d} -> {len(names):3d}  |out| {o64.abs().max().item():9.3e}  err32_out {e_out:9.3e}  "
              f"|grad| {g64.abs().max().item():9.3e}  err32_grad {e_grad:9.3e}")
    path = os.path.join(ROOT, "tests", "golden", "constraints.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB, {len(CASES)} cases")


if __name__ == "__main__":
    main()
