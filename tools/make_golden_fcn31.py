"""Record values of the reference's FourCastNet3.1 building blocks for tests/golden/ (data only: inputs, weights, outputs).

The reference's own classes are imported through ``oracle.ref_shims`` at generation time only (a checkout of the reference at
``MAKANI_REFERENCE_ROOT``); nothing of it is needed to run the tests.  Written: ``tests/golden/imputation.npz``, a handful of fp32
cases of ``MLPImputation`` and ``ConstantImputation`` (forward, input gradient, parameter gradients), which pin the fp64
restatement of tests/_impute_ref.py (tests/test_imputation.py); and three fixtures of the reference's own
``AtmoSphericNeuralOperatorNet31`` over the restated torch-harmonics operators of ``oracle/`` in the format of
``fcn3_small_33x64.npz`` (kwargs, ``x`` with NaN, ``g``, ``y``, ``gx``, ``param/*``, ``grad/*``, and the index buffers as
``buffer/*``).  The shimmed DISCO class is wrapped to accept and drop ``fused=``.

    python tools/make_golden_fcn31.py [--out tests/golden] [imputation] [network]"""
import argparse
import json
import os
import sys

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shims          # noqa: E402


class Sin(nn.Module):
    def forward(self, x):
        return torch.sin(x)


ACTS = {"gelu": nn.GELU, "relu": nn.ReLU, "silu": nn.SiLU, "sin": Sin}

# name: (shape, imputed channels, mask planes (None | 1 | "ni"), mlp_ratio, activation)
MLP_CASES = {
    "mlp_gelu_nan_only": ((2, 4, 5, 6), [1], None, 2.0, "gelu"),
    "mlp_relu_mask_ni": ((2, 5, 4, 6), [4, 0], "ni", 2.0, "relu"),
    "mlp_silu_mask_1": ((1, 6, 5, 4), [2, 5, 3], 1, 1.0, "silu"),
    "mlp_sin_leading_dims": ((2, 2, 3, 4, 5), [0], "ni", 3.0, "sin"),
}
# name: (shape, mask shape | None)
CONST_CASES = {
    "const_nan_only": ((2, 3, 4, 5), None),
    "const_mask_plane": ((2, 3, 4, 5), (1, 1, 4, 5)),
    "const_mask_full": ((1, 2, 4, 3, 5), (1, 2, 4, 3, 5)),
}


def imputation_cases():
    """{key: array} of every case: inputs with NaN, mask, parameters, output, gradients of sum(y * g), and a json description"""
    mod = ref_shims.import_reference_module("makani.models.common.imputation")
    out = {}
    gen = torch.Generator().manual_seed(31)
    for name, (shape, imp, planes, ratio, act) in MLP_CASES.items():
        C, NI = shape[-3], len(imp)
        m = mod.MLPImputation(inp_chans=C, inpute_chans=torch.tensor(imp), mlp_ratio=ratio, activation_function=ACTS[act])
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
        x = torch.randn(shape, generator=gen)
        sub = (*shape[:-3], NI, *shape[-2:])
        x[..., imp, :, :] = torch.where(torch.rand(sub, generator=gen) < 0.25, torch.full((), float("nan")), x[..., imp, :, :])
        mask = None
        if planes is not None:
            mask = torch.rand((*shape[:-3], NI if planes == "ni" else 1, *shape[-2:]), generator=gen) < 0.3
        g = torch.randn(shape, generator=gen)
        xr = x.clone().requires_grad_(True)
        y = m(xr, mask)
        params = dict(m.named_parameters())
        grads = torch.autograd.grad(y, [xr, *params.values()], g)
        out[f"{name}/meta"] = np.array(json.dumps(dict(imp=imp, mlp_ratio=ratio, act=act, has_mask=mask is not None)))
        out.update({f"{name}/x": x.numpy(), f"{name}/g": g.numpy(), f"{name}/y": y.detach().numpy(), f"{name}/gx": grads[0].numpy()})
        if mask is not None:
            out[f"{name}/mask"] = mask.numpy()
        for (k, p), gp in zip(params.items(), grads[1:]):
            out[f"{name}/param/{k}"] = p.detach().numpy()
            out[f"{name}/grad/{k}"] = gp.numpy()
    for name, (shape, mshape) in CONST_CASES.items():
        m = mod.ConstantImputation(inp_chans=shape[-3])
        with torch.no_grad():
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
        x = torch.randn(shape, generator=gen)
        x = torch.where(torch.rand(shape, generator=gen) < 0.25, torch.full((), float("nan")), x)
        mask = None if mshape is None else torch.rand(mshape, generator=gen) < 0.3
        g = torch.randn(shape, generator=gen)
        xr = x.clone().requires_grad_(True)
        y = m(xr, mask)
        gx, gw = torch.autograd.grad(y, [xr, m.weight], g)
        out[f"{name}/meta"] = np.array(json.dumps(dict(has_mask=mask is not None)))
        out.update({f"{name}/x": x.numpy(), f"{name}/g": g.numpy(), f"{name}/y": y.detach().numpy(), f"{name}/gx": gx.numpy(),
                    f"{name}/param/weight": m.weight.detach().numpy(), f"{name}/grad/weight": gw.numpy()})
        if mask is not None:
            out[f"{name}/mask"] = mask.numpy()
    return out


CHANS = ["u500", "v500", "t500", "q500", "u850", "v850", "t850", "q850", "u10m", "v10m", "t2m", "tcwv"]
NETWORK_CASES = {
    # name: (batch, seed, kwargs)
    "fcn31_small_33x64": (1, 3101, dict(
        inp_shape=(33, 64), out_shape=(33, 64), scale_factor=2, filter_basis_type="morlet", channel_names=CHANS + ["sst"],
        aux_channel_names=["xzen", "xoro", "xlsml"], pos_embed_dim=2, normalization_layer="instance_norm", big_skip=True,
        clamp_water=True, num_layers=4, sfno_block_frequency=2, embed_dim=16, aux_embed_dim=4, hard_thresholding_fraction=1.0)),
    "fcn31_history_24x48": (2, 3102, dict(
        inp_shape=(24, 48), out_shape=(24, 48), scale_factor=2, filter_basis_type="morlet", channel_names=CHANS[:8] + ["t2m", "sst"],
        aux_channel_names=["xzen", "xoro"], n_history=1, pos_embed_dim=0, normalization_layer="layer_norm", activation_function="sin",
        encoder_bias=True, num_layers=2, embed_dim=8, aux_embed_dim=4, hard_thresholding_fraction=1.0, big_skip=True)),
    "fcn31_nomlp_24x48": (1, 3103, dict(
        inp_shape=(24, 48), out_shape=(24, 48), scale_factor=2, filter_basis_type="morlet", channel_names=CHANS,
        aux_channel_names=["xzen"], use_mlp=False, layer_scale=False, resample_sht=True, clamp_water=True, num_layers=3,
        embed_dim=8, aux_embed_dim=4, hard_thresholding_fraction=1.0, normalization_layer="none",
        normalization_means=[0.1 * (i % 5) - 0.2 for i in range(12)], normalization_stds=[0.5 + 0.125 * (i % 4) for i in range(12)])),
}


def reference_network():
    """the reference's ``AtmoSphericNeuralOperatorNet31`` over the oracle's operators; the DISCO class drops ``fused=``"""
    ref_shims.install()
    th = sys.modules["torch_harmonics"]
    base = th.DiscreteContinuousConvS2
    if not getattr(base, "_drops_fused", False):
        class DiscreteContinuousConvS2(base):
            _drops_fused = True

            def __init__(self, *a, fused=None, **k):
                super().__init__(*a, **k)
        th.DiscreteContinuousConvS2 = DiscreteContinuousConvS2
    return ref_shims.import_reference_module("makani.models.networks.fourcastnet3_1").AtmoSphericNeuralOperatorNet31


def network_inputs(name):
    """(x with NaN in the sst channels and a fractional land mask where the network has one, g) of a case, seeded"""
    batch, seed, kw = NETWORK_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    names, aux, nh = kw["channel_names"], kw["aux_channel_names"], kw.get("n_history", 0)
    dyn = [a for a in aux if a not in ("xoro", "xlsml", "xlsms")]
    n_dyn = len(names) + len(dyn)
    nin = n_dyn * (nh + 1) + (len(aux) - len(dyn))
    x = torch.rand(batch, nin, *kw["inp_shape"], generator=gen)
    if "xlsml" in aux:
        u = torch.rand(batch, *kw["inp_shape"], generator=gen)
        x[:, len(names) + aux.index("xlsml")] = torch.where(u < 0.6, torch.zeros(()), (u - 0.6) / 0.4)
    if "sst" in names:
        for ih in range(nh + 1):
            c = names.index("sst") + ih * n_dyn
            x[:, c] = torch.where(torch.rand(batch, *kw["inp_shape"], generator=gen) < 0.3, torch.full((), float("nan")), x[:, c])
    g = torch.randn(batch, len(names), *kw["out_shape"], generator=gen)
    return x, g


def network_case(name):
    batch, seed, kw = NETWORK_CASES[name]
    torch.manual_seed(seed)
    model = reference_network()(**kw)
    model.train()
    with torch.no_grad():          # the embedding starts at zero: give it values
        if hasattr(model, "pos_embed"):
            model.pos_embed.position_embeddings.normal_(0.0, 0.5)
    x, g = network_inputs(name)
    xr = x.clone().requires_grad_(True)
    y = model(xr)
    (y * g).sum().backward()
    assert torch.isfinite(y).all() and torch.isfinite(xr.grad).all()
    rec = {"kwargs": np.array(json.dumps(kw)), "x": x.numpy(), "g": g.numpy(), "y": y.detach().numpy(), "gx": xr.grad.numpy()}
    for k, v in model.state_dict().items():
        rec["param/" + k] = v.detach().numpy()
    for k, p in model.named_parameters():
        rec["grad/" + k] = p.grad.numpy()
    for k, b in model.named_buffers():
        if k.endswith("_channels") or k.endswith("_channels_in") or k.endswith("_channels_out"):
            rec["buffer/" + k] = b.numpy()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("which", nargs="*", default=["imputation", "network"])
    a = ap.parse_args()
    if not ref_shims.reference_available():
        raise SystemExit(f"no reference checkout at {ref_shims.REFERENCE_ROOT} (set MAKANI_REFERENCE_ROOT)")
    if "imputation" in a.which:
        path = os.path.join(a.out, "imputation.npz")
        np.savez_compressed(path, **imputation_cases())
        print(path, os.path.getsize(path), "bytes")
    if "network" in a.which:
        for name in NETWORK_CASES:
            path = os.path.join(a.out, name + ".npz")
            rec = network_case(name)
            np.savez_compressed(path, **rec)
            print(path, os.path.getsize(path), "bytes", len([k for k in rec if k.startswith("param/")]), "state-dict keys")


if __name__ == "__main__":
    main()
