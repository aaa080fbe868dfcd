"""Record tests/golden/metricshandler.npz: the reference's own, unmodified ``MetricsHandler`` (makani/utils/metric.py), imported
through oracle.ref_shims and run in fp32 on the CPU.  ``params`` is a ``ParamsBase`` with ``normalization="zscore"``; the
normalisation fields are ``.npy`` files in a temporary directory.  Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from
the repository root:  python tools/make_metricshandler_golden.py

Only data is recorded.  Per case: the configuration (JSON), every call's inputs as int8 (prediction, target, climatology: times
2^-5; weight: times 2^-6; NaN targets as an int8 mask), every handle's curve and counter after each ``update``, the finalized
curves, the ACC integral and the scalar entries of ``logs`` (keys as JSON, values as an array).  All cases: 9 x 16 points, 11
channels, B = 2, three rollout steps.

The inputs are conditioned so that the reference's fp32 arithmetic is itself accurate to better than 1e-6: members = a common
field + small member noise, the target = the common field + noise (anomalies correlate, skill exceeds spread / E)."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, B, STEPS = 9, 16, 2, 3
NAMES = "u10m t2m sp sst u500 z500 q500 q50 t850 v10m z850".split()
C = len(NAMES)
SHIFT, WSHIFT = 5, 6

LISTS = dict(l1_var_names=["z500", "u10m", "q50"], rmse_var_names=["t2m", "z500", "sst", "u10m"], acc_var_names=["z500", "t850", "u500"],
             crps_var_names=["q500", "z500"], spread_var_names=["z500", "sp", "z850", "t2m"], ssr_var_names=["v10m", "z500"],
             rh_var_names=["z500", "q50"])
DET = dict(LISTS, crps_var_names=[], spread_var_names=[], ssr_var_names=[], rh_var_names=[])
ABSENT = dict(LISTS, l1_var_names=["z500", "w300", "u10m"], rh_var_names=["tcwv", "z500"])

# name, ensemble size, handler kwargs, passes over the three steps, weights, (pass, channel, sample) of NaN targets | None,
# with a climatology, model_grid_type
CASES = [
    ("full", 3, LISTS, 2, False, None, True),
    ("deterministic", 1, DET, 1, False, None, True),
    ("weights", 3, LISTS, 1, True, None, True),
    ("nan", 3, LISTS, 2, False, (1, NAMES.index("z500"), 1), True),
    ("wb2", 3, dict(LISTS, wb2_compatible=True), 1, False, None, True),
    ("noclim", 3, LISTS, 1, False, None, False),
    ("absent", 3, ABSENT, 1, False, None, True),
]


def q8(t, shift=SHIFT):
    return torch.clamp(torch.round((2 ** shift) * t), -127, 127).to(torch.int8)


def main():
    from oracle import ref_shims
    ref_shims.install()
    metric_mod = ref_shims.import_reference_module("makani.utils.metric")
    yp = ref_shims.import_reference_module("makani.utils.YParams")
    gen = torch.Generator().manual_seed(4711)
    scale = np.linspace(0.5, 3.0, C, dtype=np.float32).reshape(1, C, 1, 1)
    bias = np.linspace(-1.0, 1.0, C, dtype=np.float32).reshape(1, C, 1, 1)
    out = {"scale": scale}
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "means.npy"), bias)
        np.save(os.path.join(tmp, "stds.npy"), scale)
        for name, E, hkw, passes, with_w, nan_at, with_clim in CASES:
            params = yp.ParamsBase()
            cfg = dict(log_to_screen=False, log_to_wandb=False, channel_names=NAMES, dt=1, dhours=6, split_data_channels=False,
                       out_channels=list(range(C)), N_out_channels=C, img_shape_x_resampled=H, img_shape_y_resampled=W,
                       img_crop_offset_x=0, img_crop_offset_y=0, model_grid_type="equiangular", ensemble_size=E)
            params.update_params(dict(cfg, normalization="zscore", global_means_path=os.path.join(tmp, "means.npy"),
                                      global_stds_path=os.path.join(tmp, "stds.npy")))
            ci = q8(0.5 * torch.randn(1, C, H, W, generator=gen))
            clim = ci.float() / 2 ** SHIFT if with_clim else None
            handler = metric_mod.MetricsHandler(params, clim, STEPS, torch.device("cpu"), **hkw)
            handler.initialize_buffers()
            handler.zero_buffers()
            if with_clim:
                out[f"{name}/clim"] = ci.numpy()
            call = 0
            for ip in range(passes):
                for idt in range(STEPS):
                    common = 1.5 * torch.randn(B, C, H, W, generator=gen)
                    member = 0.4 * torch.randn(B, E, C, H, W, generator=gen) + 0.25 * (torch.arange(E) - 0.5 * (E - 1)).reshape(1, E, 1, 1, 1)
                    pi = q8(common.unsqueeze(1) + member)
                    ti = q8(common + 0.8 * torch.randn(B, C, H, W, generator=gen))
                    prd, tar = pi.float() / 2 ** SHIFT, ti.float() / 2 ** SHIFT
                    if E == 1:
                        prd = prd[:, 0]
                    out[f"{name}/call{call}/prd"] = pi.numpy()
                    out[f"{name}/call{call}/tar"] = ti.numpy()
                    wgt = None
                    if with_w:
                        wi = torch.randint(16, 128, (B, C, H, W), generator=gen).to(torch.int8)
                        out[f"{name}/call{call}/wgt"] = wi.numpy()
                        wgt = wi.float() / 2 ** WSHIFT
                    if nan_at is not None and nan_at[0] == ip:
                        mask = torch.zeros(B, C, H, W, dtype=torch.int8)
                        mask[nan_at[2], nan_at[1]] = (torch.rand(H, W, generator=gen) < 0.3).to(torch.int8)
                        out[f"{name}/call{call}/nan"] = mask.numpy()
                        tar = torch.where(mask > 0, torch.full_like(tar, float("nan")), tar)
                    loss = torch.tensor(0.25 * (call + 1))
                    handler.update(prd, tar, loss, idt, wgt)
                    for h in handler.metric_handles:
                        out[f"{name}/call{call}/{h.metric_name}/curve"] = h.rollout_curve.detach().clone().numpy()
                        out[f"{name}/call{call}/{h.metric_name}/counter"] = h.rollout_counter.detach().clone().numpy()
                    call += 1
            logs = handler.finalize()
            for h in handler.metric_handles:
                out[f"{name}/final/{h.metric_name}"] = h.rollout_curve_cpu.clone().numpy()
                if h.integrate:
                    out[f"{name}/integral/{h.metric_name}"] = h.rollout_integral_cpu.clone().numpy()
            keys = [k for k in logs["metrics"] if k != "rollouts"]
            out[f"{name}/logs"] = np.asarray([logs["base"]["validation steps"], logs["base"]["validation loss"]]
                                             + [float(logs["metrics"][k]) for k in keys], dtype=np.float64)
            meta = dict(cfg, E=E, handler_kwargs=hkw, passes=passes, calls=call, steps=STEPS, weights=with_w, climatology=with_clim,
                        shift=SHIFT, wshift=WSHIFT, log_keys=keys, dtxdh=handler.dtxdh, dd=handler.dd,
                        handles=[dict(name=h.metric_name, channels=list(h.metric_channels), curve=list(h.rollout_curve.shape),
                                      counter=list(h.rollout_counter.shape)) for h in handler.metric_handles])
            out[f"{name}/meta"] = np.array(json.dumps(meta))
            print(f"{name:14s} E {E} calls {call} handles {[h.metric_name for h in handler.metric_handles]} log entries {len(keys)}")
    path = os.path.join(ROOT, "tests", "golden", "metricshandler.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB, {len(CASES)} cases")


if __name__ == "__main__":
    main()
