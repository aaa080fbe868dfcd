"""Record tests/golden/losshandler.npz: the reference's own, unmodified ``LossHandler`` (makani/utils/loss.py),
``HydrostaticBalanceLoss`` and ``DriftRegularization``, imported through oracle.ref_shims and run in fp32 on the CPU with
``compile=False``.  ``params`` is a ``ParamsBase``; the normalisation fields are ``.npy`` files in a temporary directory.
Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_losshandler_golden.py

One wrapper, part of this tool and not of the fixture: the reference's ``HydrostaticBalanceLoss.compute_channel_weighting`` lacks
the ``time_diff_scale`` keyword that its ``LossHandler`` passes, so a handler with a "hydrostatic" entry dies with a ``TypeError``
at construction; the method is wrapped to swallow the keyword (it is None in every case here).

Per case: the configuration (JSON), every call's inputs as int8 times 2^-5 (exact in bf16, fp32 and fp64), the scalar, the
per-loss vectors, the gradient with respect to ``prd``, and the buffers (before and after the recorded call where they move).
All cases: 9 x 16 points, 11 channels, B = 2, E = 3."""
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, B, E = 9, 16, 2, 3
NAMES = "u10m t2m z500 z850 z1000 t500 t850 t1000 q500 q850 q1000".split()
C = len(NAMES)
SURFACE = {"u10m": (0.5, 5.0), "t2m": (278.0, 21.0)}
SHIFT = 5          # inputs are int8 * 2^-SHIFT


def stats():
    """normalisation statistics of realistic size: (1, C, 1, 1) bias and scale, (C) standard deviations of the time difference"""
    bias, scale = [], []
    for n in NAMES:
        if n in SURFACE:
            b, s = SURFACE[n]
        else:
            k = math.log(1000.0 / int(n[1:])) / math.log(20.0)
            b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3 * (0.8 + 0.4 * k)), "t": (285.0 - 70.0 * k, 15.0 - 6.0 * k),
                    "q": (2.0e-3 * (1.0 - k) ** 3 + 2e-6, 2.0e-3 * (1.0 - k) ** 3 + 1e-6)}[n[0]]
        bias.append(b)
        scale.append(s)
    bias = np.asarray(bias, dtype=np.float32).reshape(1, C, 1, 1)
    scale = np.asarray(scale, dtype=np.float32).reshape(1, C, 1, 1)
    tds = (scale.reshape(-1) * np.linspace(0.2, 0.7, C)).astype(np.float32)
    return bias, scale, tds


L2 = {"type": "l2", "channel_weights": "auto", "temp_diff_normalization": True}
CRPS = {"type": "ensemble_crps", "relative_weight": 0.5}
DRIFT = {"type": "drift_regularization", "parameters": {"p": 2}}


def hydro(moist):
    return {"type": "hydrostatic", "parameters": {"p_min": 400, "use_moist_air_formula": moist}, "relative_weight": 1e-4}


# name, params entries, handler kwargs, training, number of calls (the last one is recorded), with an input state
CASES = [
    ("l2_eval", dict(losses=[{"type": "l2"}], n_future=0), {}, False, 1, False),
    ("multistep", dict(losses=[L2, CRPS, DRIFT], n_future=1, multistep={"weight_type": "linear"}), {}, True, 1, False),
    ("mixed_dry", dict(losses=[L2, dict(CRPS, tendency=True), DRIFT, hydro(False)], n_future=0), {}, True, 1, True),
    ("mixed_moist", dict(losses=[L2, dict(CRPS, tendency=True), DRIFT, hydro(True)], n_future=0), {}, True, 1, True),
    ("balanced", dict(losses=[{"type": "l2"}, CRPS], n_future=0, balanced_weighting=True), {}, True, 102, False),
    ("running_stats", dict(losses=[{"type": "l2"}, CRPS], n_future=0), dict(track_running_stats=True), True, 2, False),
]


def quantised(shape, gen):
    return torch.clamp(torch.round((2 ** SHIFT) * torch.randn(*shape, generator=gen)), -127, 127).to(torch.int8)


def main():
    from oracle import ref_shims
    ref_shims.install()
    loss_mod = ref_shims.import_reference_module("makani.utils.loss")
    hyd_mod = ref_shims.import_reference_module("makani.utils.losses.hydrostatic_loss")
    yp = ref_shims.import_reference_module("makani.utils.YParams")
    own = hyd_mod.HydrostaticBalanceLoss.compute_channel_weighting

    def swallowing(self, channel_weight_type, time_diff_scale=None):
        assert time_diff_scale is None
        return own(self, channel_weight_type)

    hyd_mod.HydrostaticBalanceLoss.compute_channel_weighting = swallowing
    bias, scale, tds = stats()
    gen = torch.Generator().manual_seed(2031)
    out = {"bias": bias, "scale": scale, "time_diff_stds": tds}
    with tempfile.TemporaryDirectory() as tmp:
        for n, a in (("means", bias), ("stds", scale), ("tds", tds)):
            np.save(os.path.join(tmp, n + ".npy"), a)
        for name, entries, hkw, training, calls, with_inp in CASES:
            params = yp.ParamsBase()
            cfg = dict(n_history=1 if with_inp else 0, img_shape_x_resampled=H, img_shape_y_resampled=W, img_crop_offset_x=0,
                       img_crop_offset_y=0, channel_names=NAMES, out_channels=list(range(C)), model_grid_type="equiangular",
                       normalization="zscore", global_means_path=os.path.join(tmp, "means.npy"),
                       global_stds_path=os.path.join(tmp, "stds.npy"), time_diff_stds_path=os.path.join(tmp, "tds.npy"), **entries)
            params.update_params(cfg)
            handler = loss_mod.LossHandler(params, compile=False, **hkw).train(training)
            S = entries["n_future"] + 1
            vectors = []
            hooks = [fn.register_forward_hook(lambda m, i, o: vectors.append(o.detach().clone())) for fn in handler.loss_fn]
            for call in range(calls):
                last = call == calls - 1
                if last:
                    for k, v in handler.state_dict().items():
                        out[f"{name}/before/{k}"] = v.detach().clone().numpy()
                pi, ti = quantised((B, E, S * C, H, W), gen), quantised((B, S * C, H, W), gen)
                ii = quantised((B, 2 * C, H, W), gen) if with_inp else None
                prd = (pi.float() / 2 ** SHIFT).requires_grad_(True)
                tar = ti.float() / 2 ** SHIFT
                inp = ii.float() / 2 ** SHIFT if with_inp else None
                del vectors[:]
                loss = handler(prd, tar, None, inp)
                if last or name == "running_stats":
                    out[f"{name}/call{call if not last else 'R'}/prd"] = pi.numpy()
                    out[f"{name}/call{call if not last else 'R'}/tar"] = ti.numpy()
                    if with_inp:
                        out[f"{name}/call{call if not last else 'R'}/inp"] = ii.numpy()
            (grad,) = torch.autograd.grad(loss, prd)
            for h in hooks:
                h.remove()
            out[f"{name}/loss"] = loss.detach().numpy()
            out[f"{name}/grad"] = grad.numpy()
            for i, v in enumerate(vectors):
                out[f"{name}/vec{i}"] = v.numpy()
            for k, v in handler.named_buffers():
                if k.split(".")[-1] in ("channel_weights", "multistep_weight", "running_mean", "running_var", "num_batches_tracked", "cmat", "p"):
                    out[f"{name}/buf/{k}"] = v.detach().clone().numpy()
            meta = dict(cfg, training=training, calls=calls, handler_kwargs=hkw, with_inp=with_inp, persistent=sorted(handler.state_dict()),
                        loss_types=[int(t) for t in handler.loss_types], shift=SHIFT)
            for k in ("global_means_path", "global_stds_path", "time_diff_stds_path"):
                del meta[k]
            out[f"{name}/meta"] = np.array(json.dumps(meta))
            print(f"{name:14s} loss {loss.item():.8e}  |grad| {grad.abs().max().item():.3e}  vectors {[tuple(v.shape) for v in vectors]}")
    path = os.path.join(ROOT, "tests", "golden", "losshandler.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB, {len(CASES)} cases")


if __name__ == "__main__":
    main()
