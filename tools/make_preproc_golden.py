"""Record tests/golden/preproc.npz from the reference's own, unmodified ``Preprocessor2D`` (makani/models/preprocessor.py),
imported through oracle.ref_shims and run on the CPU.  9 x 16 equiangular grid, B = 2, C = 3 data and U = 2 unpredicted channels;
the inputs are drawn from seeds by tests/_preproc_ref.py (``seeded_field`` / ``seeded``: |mu| / sigma <= 3, no constant channel)
and are not stored.  Cases: history_normalization_mode none | mean | exponential (decay 0.5) x n_history 0 | 2, each plain and
with ``add_grid`` (two frequencies, with cos), one file-backed static plane (``add_orography``) and a bias field.  Per case: the
assembled network input, history_mean / history_std, the de-normalised prediction of a seeded yn, the gradients of
sum(out r1) + sum(y r2) w.r.t. window and yn, and one ``append_history`` step with the slide of the cached unpredicted input.

The file readers of makani/utils/auxiliary_fields.py need h5py; this process installs an inert stand-in module that returns seeded
arrays instead (the reference still does its own normalisation of the orography and its own slicing of the bias field), and the
all-reduce of a one-rank spatial group, which the shim leaves out, is the identity.  Nothing
under oracle/ is edited.  Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:
    python tools/make_preproc_golden.py"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

H, W, B, C, U = 9, 16, 2, 3, 2
MODES = ("none", "mean", "exponential")


class Params(dict):
    """the attribute / ``get`` access of makani's parameter object"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def case_params(mode, nh, rich):
    p = Params(img_shape_x=H, img_shape_y=W, img_shape_x_resampled=H, img_shape_y_resampled=W, n_history=nh,
               history_normalization_mode=mode, model_grid_type="equiangular", data_grid_type="equiangular", out_channels=C)
    if mode == "exponential":
        p["history_normalization_decay"] = 0.5
    if rich:
        p.update(add_grid=True, gridtype="sinusoidal", grid_num_frequencies=2, add_cos_to_grid=True, add_orography=True,
                 orography_path=os.path.abspath(__file__), bias_correction=os.path.abspath(__file__))
    return p


def seeds(mode, nh, rich):
    base = 1000 * (MODES.index(mode) + 1) + 100 * nh + 10 * int(rich)
    return dict(win=base + 1, xz=base + 2, yz=base + 3, yn=base + 4, r1=base + 5, r2=base + 6)


def main():
    from oracle import ref_shims
    import _preproc_ref as R
    ref_shims.install()
    aux = types.ModuleType("makani.utils.auxiliary_fields")
    aux.get_orography = lambda path: R.seeded((H, W), 71, mean=300.0, std=500.0).float().numpy()
    aux.get_bias_correction = lambda path, out_channels: (0.2 * R.seeded((1, C, H, W), 72)).float().numpy()
    sys.modules["makani.utils.auxiliary_fields"] = aux
    mod = ref_shims.import_reference_module("makani.models.preprocessor")
    # copy_to_parallel_region's backward all-reduces over the spatial group; the shim leaves the collective out.  One rank: identity.
    import makani.mpu.mappings as mappings
    mappings._reduce = lambda t, group=None: t
    out = {}
    for mode in MODES:
        for nh in (0, 2):
            for rich in (False, True):
                name = f"{mode}_h{nh}_{'rich' if rich else 'plain'}"
                T, sd = nh + 1, seeds(mode, nh, rich)
                P = mod.Preprocessor2D(case_params(mode, nh, rich))
                P.train()
                win = R.seeded_field((B, T, C, H, W), sd["win"]).float().flatten(1, 2).requires_grad_(True)
                xz = R.seeded_field((B, T, U, H, W), sd["xz"]).float()
                yz = R.seeded_field((B, 2, U, H, W), sd["yz"]).float()
                P.cache_unpredicted_features(None, None, xz, yz)
                inpa = P.append_unpredicted_features(win)
                P.history_compute_stats(inpa)
                net_in = P.add_static_features(P.history_normalize(inpa, target=False))
                yn = R.seeded((B, C, H, W), sd["yn"]).float().requires_grad_(True)
                y = P.history_denormalize(P.correct_bias(yn), target=True)
                r1, r2 = R.seeded(net_in.shape, sd["r1"]).float(), R.seeded(y.shape, sd["r2"]).float()
                gwin, gyn = torch.autograd.grad((net_in * r1).sum() + (y * r2).sum(), [win, yn])
                nxt = P.append_history(win.detach(), y.detach(), 0)
                meta = dict(mode=mode, n_history=nh, rich=rich, seeds=sd, B=B, C=C, U=U, img_shape=[H, W],
                            params={k: v for k, v in case_params(mode, nh, rich).items() if not k.endswith("path") and k != "bias_correction"})
                out[f"{name}/meta"] = np.array(json.dumps(meta))
                if rich:
                    out[f"{name}/static"] = P.static_features.numpy().copy()
                    out[f"{name}/bias"] = P.bias_correction.numpy().copy()
                for key, t in (("out", net_in), ("history_mean", P.history_mean), ("history_std", P.history_std), ("y", y), ("gwin", gwin),
                               ("gyn", gyn), ("next_window", nxt), ("next_unpredicted", P.unpredicted_inp_train)):
                    out[f"{name}/{key}"] = t.detach().numpy().copy()
                # cross-check against the fp64 restatement before anything is written
                q, wt = R.quad_weights(H, W), (None if mode == "none" else R.time_weights(mode, nh, 0.5))
                stat = P.static_features[0].double() if rich else None
                want, mu, sigma = R.assemble(win.detach().double(), xz.double(), None, stat, T, mode, q, wt)
                err = R.rel(net_in, want)
                assert err < 1e-5, (name, err)
                assert mode == "none" or float((mu.abs() / sigma).max()) <= 3.0, (name, "inputs are to have |mu| / sigma <= 3")
                print(name, tuple(net_in.shape), f"restatement {err:.1e}")
    path = os.path.join(ROOT, "tests", "golden", "preproc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
