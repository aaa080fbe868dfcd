"""Record tests/golden/interpolant.npz from the reference's own, unmodified ``StochasticInterpolantWrapper``
(makani/models/stochastic_interpolant.py), imported through oracle.ref_shims and run on the CPU with TORCHDYNAMO_DISABLE=1.
9 x 16 equiangular grid, B = 2, C = 3; the network is the stub ``Conv2d(inp_chans, C, 1)`` with seeded weights; the inputs are
drawn from seeds by tests/_preproc_ref.py (``seeded``) and are not stored.

Cases: noise_epsilon 1.0 | 0.7 x Foellmer off | on x antithetic off | on, half of them with features (U = 2 unpredicted channels,
St = 2 static planes: the reference's linear ``add_grid``; the sampler then runs at B = 1, the only batch size the reference's
``cat`` of the static planes allows), and one time-aware case.  Per case, captured by wrapping the instance's ``stochastic_path``
and ``noise_module.forward`` and by a forward pre-hook of the stub:

    s (B, S') and the noise field of the training call (n_samples = 3), the per-step noise fields of the samplers (n_steps 1, 3)
    from a second run of the class in float64 fed the same times and noise: the x slot of the network input, the drift target,
    the predicted drift (cases without antithetic pairs), the samplers' results
    err32_*: the largest distance between the class's float32 and float64 runs, per quantity

What is NOT stored, to keep the file under 1 MiB: the copied slots of the network input (x0, xu, static, s plane: checked here
bit for bit against the seeded inputs, the recorded static planes and s before anything is written, and rebuilt by the tests), the
predicted drift of the cases with antithetic pairs (the stub is linear in the network input), and the float32 runs themselves
(only their distances err32_* from the float64 runs).

The float64 run and the fp64 restatement tests/_interp_ref.py are compared here before anything is written.  Nothing under
oracle/ is edited.  Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository root:
    python tools/make_interpolant_golden.py"""
import json
import os
import sys

os.environ["TORCHDYNAMO_DISABLE"] = "1"

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

H, W, B, C, U, ST, NS = 9, 16, 2, 3, 2, 2, 3
STEPS = (1, 3)


class Params(dict):
    """the attribute / ``get`` access of makani's parameter object"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def case_params(feat, time_aware):
    p = Params(img_shape_x=H, img_shape_y=W, img_shape_x_resampled=H, img_shape_y_resampled=W, img_crop_shape_x=H, img_crop_shape_y=W,
               n_history=0, n_future=0, history_normalization_mode="none", model_grid_type="equiangular", data_grid_type="equiangular",
               N_in_predicted_channels=C, N_out_channels=C, N_static_channels=ST if feat else 0, N_dynamic_channels=U if feat else 0,
               batch_size=B, time_aware=time_aware, out_channels=C)
    if feat:
        p.update(add_grid=True, gridtype="linear")
    return p


class Stub(torch.nn.Module):
    """Conv2d(inp_chans, C, 1); the time-aware form hands it the time as a second argument, which it ignores"""

    def __init__(self, inp_chans, seed):
        import _preproc_ref as R
        super().__init__()
        self.conv = torch.nn.Conv2d(inp_chans, C, 1)
        with torch.no_grad():
            self.conv.weight.copy_(0.3 * R.seeded(self.conv.weight.shape, seed))
            self.conv.bias.copy_(0.1 * R.seeded(self.conv.bias.shape, seed + 1))

    def forward(self, x, s=None):
        return self.conv(x)


class Capture:
    """what one forward of the wrapper saw: the arguments of stochastic_path, every noise draw, every network input"""

    def __init__(self, wrapper, replay=None):
        self.path, self.noise, self.net_in, self.net_s = [], [], [], []
        self.replay = None if replay is None else list(replay)
        path, noise = wrapper.stochastic_path, wrapper.noise_module.forward

        def path_w(x0, x1, z, s, **kw):
            self.path.append((s.detach().clone(), z.detach().clone()))
            return path(x0, x1, z, s, **kw)

        def noise_w(*a, **kw):
            out = noise(*a, **kw)
            if self.replay is not None:          # the float64 run sees the float32 run's draws
                out = self.replay.pop(0).to(torch.float64).reshape(out.shape)
            self.noise.append(out.detach().clone())
            return out

        wrapper.stochastic_path, wrapper.noise_module.forward = path_w, noise_w
        self.hook = wrapper.model.model.register_forward_pre_hook(
            lambda m, args: (self.net_in.append(args[0].detach().clone()), self.net_s.append(args[1].detach().clone() if len(args) > 1 else None))
            and None)
        self.undo = lambda: (setattr(wrapper, "stochastic_path", path), setattr(wrapper.noise_module, "forward", noise), self.hook.remove())


class FixedUniform:
    """``Tensor.uniform_`` fills with the given times instead: the float64 run of the class uses the float32 run's draw"""

    def __init__(self, s):
        self.s = s

    def __enter__(self):
        self.orig = torch.Tensor.uniform_
        s = self.s
        torch.Tensor.uniform_ = lambda t, *a, **k: t.copy_(s.to(t.dtype).reshape(t.shape))

    def __exit__(self, *exc):
        torch.Tensor.uniform_ = self.orig


def main():
    from oracle import ref_shims
    import _interp_ref as I
    import _preproc_ref as R
    ref_shims.install()
    mod = ref_shims.import_reference_module("makani.models.stochastic_interpolant")
    out = {}
    cases = [(eps, f, a, bool(f) != bool(a), False) for eps in (1.0, 0.7) for f in (0, 1) for a in (0, 1)] + [(0.7, 1, 1, True, True)]
    for idx, (eps, foell, anti, feat, ta) in enumerate(cases):
        name = f"e{int(round(10 * eps)):02d}_f{foell}_a{anti}_{'feat' if feat else 'plain'}" + ("_ta" if ta else "")
        sd = dict(x0=7000 + 10 * idx, x1=7001 + 10 * idx, xu=7002 + 10 * idx, net=7003 + 10 * idx)
        cin = 2 * C + (U + ST if feat else 0) + (0 if ta else 1)

        def build(dtype):
            w = mod.StochasticInterpolantWrapper(case_params(feat, ta), lambda inp_chans: Stub(inp_chans, sd["net"]), noise_epsilon=eps,
                                                 use_foellmer=bool(foell), antithetic_sampling=bool(anti), seed=333 + idx)
            assert w.model.model.conv.in_channels == cin
            return w.to(dtype) if dtype == torch.float64 else w

        x0, x1 = R.seeded((B, C, H, W), sd["x0"]).float(), R.seeded((B, C, H, W), sd["x1"]).float()
        xu = R.seeded((B, 1, U, H, W), sd["xu"]).float() if feat else None

        def cache(w, n, dtype):
            for mode in (True, False):
                w.train(mode)
                w.preprocessor.cache_unpredicted_features(None, None, None if xu is None else xu[:n].to(dtype), None)

        meta = dict(eps=eps, foellmer=bool(foell), antithetic=bool(anti), time_aware=ta, B=B, C=C, U=U if feat else 0, St=ST if feat else 0,
                    H=H, W=W, n_samples=NS, n_steps=list(STEPS), sampler_B=1 if feat else B, seeds=sd, net_scale=[0.3, 0.1])
        rec = {}
        # ---- training: float32, then float64 fed the same times and noise
        w32 = build(torch.float32)
        cache(w32, B, torch.float32)
        w32.train()
        cap = Capture(w32)
        pred32, drift32 = w32(x0, x1, n_samples=NS)
        cap.undo()
        (s, z), X32 = cap.path[0], cap.net_in[0]
        s_draw = s[:, :NS].clone()
        w64 = build(torch.float64)
        cache(w64, B, torch.float64)
        w64.train()
        cap64 = Capture(w64, replay=[z.reshape(B, 1, C, H, W)])
        with FixedUniform(s_draw):
            pred64, drift64 = w64(x0.double(), x1.double(), n_samples=NS)
        cap64.undo()
        X64 = cap64.net_in[0]
        assert torch.equal(cap64.path[0][0].float(), s) and torch.equal(cap64.path[0][1].float(), z)
        static = w32.preprocessor.static_features.detach().clone() if feat else None
        rec.update(s=s, s_draw=s_draw, z=z.reshape(B, C, H, W), x64=X64[:, C:2 * C], drift64=drift64)
        if not anti:
            rec["pred64"] = pred64
        if feat:
            rec["static"] = static
        if ta:
            assert torch.equal(cap.net_s[0], s.flatten().unsqueeze(1))
        rec["err32_x"] = (X32[:, C:2 * C].double() - X64[:, C:2 * C]).abs().max()
        rec["err32_drift"] = (drift32.double() - drift64).abs().max()
        rec["err32_pred"] = (pred32.double() - pred64).abs().max()
        # the copied slots are copies in both runs
        want_X, want_D = I.assemble(x0, x1, z.reshape(B, C, H, W), s, None if xu is None else xu[:, 0], None if static is None else static[0], eps,
                                    has_s=not ta)
        scale = max(float(want_X.abs().max()), float(want_D.abs().max()))
        assert float((want_X - X64).abs().max()) <= 1e-12 * scale and float((want_D - drift64).abs().max()) <= 1e-12 * scale, name
        assert torch.equal(X32[:, :C], x0.repeat_interleave(s.shape[1], dim=0)) and torch.equal(X32[:, 2 * C:], want_X[:, 2 * C:].float())
        # ---- the samplers
        n = meta["sampler_B"]
        for steps in STEPS:
            cache(w32, n, torch.float32)
            w32.eval()
            cap = Capture(w32)
            with torch.no_grad():
                y32 = w32(x0[:n], n_steps=steps)
            cap.undo()
            draws = [t.reshape(n, C, H, W) for t in cap.noise]
            assert len(draws) == steps
            cache(w64, n, torch.float64)
            w64.eval()
            cap64 = Capture(w64, replay=[t.reshape(n, 1, C, H, W) for t in draws])
            with torch.no_grad():
                y64 = w64(x0[:n].double(), n_steps=steps)
            cap64.undo()
            rec[f"noise_n{steps}"] = torch.stack(draws)
            rec[f"y64_n{steps}"] = y64
            rec[f"err32_y_n{steps}"] = (y32.double() - y64).abs().max()
            net = I.stub(w64.model.model.conv.weight.detach(), w64.model.model.conv.bias.detach())
            want = I.sampler(net, x0[:n], None if xu is None else xu[:n, 0], None if static is None else static[0], draws, steps, eps, bool(foell),
                             time_aware=ta)
            assert float((want - y64).abs().max()) <= 1e-12 * float(y64.abs().max()), (name, steps, float((want - y64).abs().max()))
        out[f"{name}/meta"] = np.array(json.dumps(meta))
        for key, t in rec.items():
            out[f"{name}/{key}"] = t.detach().numpy().copy()
        print(name, tuple(X32.shape), " ".join(f"{k}={float(v.detach()):.2e}" for k, v in rec.items() if k.startswith("err32")))
    path = os.path.join(ROOT, "tests", "golden", "interpolant.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
