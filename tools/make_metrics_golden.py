"""Record tests/golden/metrics.npz: the reference's own, unmodified validation metrics (makani/utils/metrics/functions.py:
GeometricL1, GeometricRMSE, GeometricACC, GeometricSpread, GeometricSSR, GeometricCRPS, GeometricRankHistogram), imported
through oracle.ref_shims and run in DOUBLE precision (modules cast with ``.double()``: the quadrature weights are the class's
fp32 values, widened; they are recorded), so that an fp64 restatement can be pinned against the record at rounding level.
Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:  python tools/make_metrics_golden.py

Per case: int8-quantised inputs (value = int8 / 4: coarse enough that members tie with each other and with the observation at
a good share of the points, so the ``side="right"`` of the rank histogram's searchsorted is exercised), optional spatial
weights and climatology, the quadrature weights, and per variant (channel_reduction, batch_reduction): the forward value
``out``, the value ``out2`` on the first input shifted by 1/4, and — where ``compute_counts`` is legal — ``counts``, the result of
``combine(stack([out, out2]), stack([counts, 2 counts]))`` and of ``finalize`` on that."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

IMG = (17, 32)
B, C = 2, 3
SCALE = 0.25
REDUCTIONS = ("none", "mean", "sum")
ALL = [(cr, br) for cr in REDUCTIONS for br in REDUCTIONS]
CROP = dict(crop_shape=[9, 20], crop_offset=[3, 5])
# name, class, kwargs, E (0: deterministic), weights, bias, variants
CASES = [
    ("l1", "GeometricL1", dict(), 0, False, False, ALL),
    ("l1_weights_normalize", "GeometricL1", dict(normalize=True), 0, True, False, [("none", "sum"), ("mean", "sum")]),
    ("rmse", "GeometricRMSE", dict(), 0, False, False, ALL),
    ("rmse_weights", "GeometricRMSE", dict(), 0, True, False, [("none", "sum"), ("sum", "sum"), ("mean", "none")]),
    ("rmse_crop_normalize", "GeometricRMSE", dict(normalize=True, **CROP), 0, False, False, [("mean", "mean")]),
    ("acc_macro", "GeometricACC", dict(), 0, False, False, ALL),
    ("acc_micro", "GeometricACC", dict(method="micro"), 0, False, False, ALL),
    ("acc_macro_bias_weights", "GeometricACC", dict(), 0, True, True, [("none", "sum"), ("mean", "sum")]),
    ("acc_micro_bias", "GeometricACC", dict(method="micro", normalize=True), 0, False, True, [("mean", "mean"), ("none", "sum")]),
    ("acc_crop_bias", "GeometricACC", dict(**CROP), 0, False, True, [("mean", "mean")]),
    ("spread_e3", "GeometricSpread", dict(), 3, False, False, ALL),
    ("spread_e2_weights", "GeometricSpread", dict(normalize=True), 2, True, False, [("none", "sum")]),
    ("spread_e1", "GeometricSpread", dict(), 1, False, False, [("none", "none")]),
    ("ssr_e3", "GeometricSSR", dict(), 3, False, False, ALL),
    ("ssr_e2_weights_crop", "GeometricSSR", dict(**CROP), 2, True, False, [("none", "sum")]),
    ("ssr_e1", "GeometricSSR", dict(), 1, False, False, [("none", "none")]),
    ("crps_e3", "GeometricCRPS", dict(crop_shape=list(IMG), crop_offset=[0, 0]), 3, False, False, ALL),
    ("crps_e2_weights", "GeometricCRPS", dict(crop_shape=list(IMG), crop_offset=[0, 0]), 2, True, False, [("none", "sum")]),
    ("crps_e1", "GeometricCRPS", dict(crop_shape=list(IMG), crop_offset=[0, 0]), 1, False, False, [("mean", "mean")]),
    ("rankhist_e3", "GeometricRankHistogram", dict(crop_shape=list(IMG), crop_offset=[0, 0]), 3, False, False, ALL),
    ("rankhist_e2_weights_normalize", "GeometricRankHistogram", dict(crop_shape=list(IMG), crop_offset=[0, 0], normalize=True), 2, True,
     False, [("none", "sum"), ("mean", "sum")]),
    ("rankhist_e1", "GeometricRankHistogram", dict(crop_shape=list(IMG), crop_offset=[0, 0]), 1, False, False, [("none", "none")]),
    ("rankhist_e3_crop", "GeometricRankHistogram", dict(**CROP), 3, False, False, [("mean", "mean")]),
]


def quantised(shape, gen):
    return torch.clamp(torch.round(torch.randn(*shape, generator=gen) / SCALE), -127, 127).to(torch.int8)


def main():
    from oracle import ref_shims
    ref_shims.install()
    # CRPSLoss scatters the spatial weights over the "ensemble" group even when it has one member; the serial shim has no
    # primitives: a split over a group of one is the identity
    maps = ref_shims.import_reference_module("makani.mpu.mappings")
    maps._split = lambda t, dim, group=None: t
    fn = ref_shims.import_reference_module("makani.utils.metrics.functions")
    out = {}
    gen = torch.Generator().manual_seed(2027)
    for name, cls, extra, E, wgt, use_bias, variants in CASES:
        shape = tuple(extra.get("crop_shape", IMG))
        lead = (B, E, C) if E else (B, C)
        aq, bq = quantised((*lead, *shape), gen), quantised((B, C, *shape), gen)
        a, b = aq.double() * SCALE, bq.double() * SCALE
        w = (torch.rand(B, C, *shape, generator=gen) + 0.5) if wgt else None
        # the climatology has the shape of the (cropped) input: functions.py:186-188 subtracts it as it is
        biasq = quantised((C, *shape), gen) if use_bias else None
        meta = dict(cls=cls, kwargs=dict(grid_type="equiangular", img_shape=list(IMG), **extra), scale=SCALE, E=E,
                    variants=[list(v) for v in variants])
        out[f"{name}/meta"] = np.array(json.dumps(meta))
        out[f"{name}/a_i8"], out[f"{name}/b_i8"] = aq.numpy(), bq.numpy()
        if w is not None:
            out[f"{name}/weights"] = w.numpy()
        if biasq is not None:
            out[f"{name}/bias_i8"] = biasq.numpy()
        for cr, br in variants:
            kw = dict(meta["kwargs"], channel_reduction=cr, batch_reduction=br)
            if biasq is not None:
                kw["bias"] = biasq.double() * SCALE
            mod = getattr(fn, cls)(**kw).double()
            out[f"{name}/quad_weight"] = mod.quadrature.quad_weight.reshape(shape).float().numpy()
            wd = w.double() if w is not None else None
            with torch.no_grad():
                val, val2 = mod(a, b, wd), mod(a + SCALE, b, wd)
            assert val.dtype == torch.float64, (name, val.dtype)
            key = f"{name}/{cr}-{br}"
            out[f"{key}/out"], out[f"{key}/out2"] = val.numpy(), val2.numpy()
            if br == "sum" or (wd is None and br == "mean"):          # (compute_counts fails otherwise: an error case of the tests)
                counts = mod.compute_counts(a, wd)
                cv, cc = mod.combine(torch.stack([val, val2], dim=0), torch.stack([counts, 2.0 * counts], dim=0), dim=0)
                out[f"{key}/counts"], out[f"{key}/comb_vals"], out[f"{key}/comb_counts"] = counts.numpy(), cv.numpy(), cc.numpy()
                out[f"{key}/final"] = mod.finalize(cv, cc).numpy()
            print(key, tuple(val.shape), val.reshape(-1)[:3].tolist())
    path = os.path.join(ROOT, "tests", "golden", "metrics.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
