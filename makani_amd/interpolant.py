"""The stochastic-interpolant stepper behind the interface of ``makani/models/stochastic_interpolant.py``: ``InterpolationWrapper``,
``TimeAwareInterpolationWrapper`` and ``StochasticInterpolantWrapper`` (Chen et al., *Probabilistic forecasting with stochastic
interpolants and Foellmer processes*), the third branch of ``get_model`` (``makani/models/model_registry.py:257-269``).

Schedule (the reference's fixed choice): alpha = 1 - s, beta = s^2, sigma = eps (1 - s), gamma = sqrt(s) sigma, d alpha = -1,
d beta = 2 s, d sigma = -eps, d gamma = -eps sqrt(s).  The network input is ``[x0 (C) | x (C) | xu (U) | static (St) | s (1)]``,
without the s plane in the time-aware form, where the network is called as ``model(x_in, s.unsqueeze(1))``.

Hot path (``csrc/interpolant.hip``), all of it affine in at most four fields with per-sample scalar coefficients:

* training, ONE launch (``mk_si_assemble``): the whole network input of the ``B S'`` rows and the drift target
  ``D = -x0 + 2 s x1 - eps sqrt(s) z`` from x0, x1, the noise field and the device tensor ``s`` — no ``repeat``, ``tile`` or
  ``cat``; every source element is read once however many time samples there are.
* sampling, ONE launch per SDE step (``mk_si_step``, with ``mk_si_step_bwd`` behind autograd): the next network input with
  ``x <- cx x + cb b + c0 x0 + cn z``, x read in place from the x slot of the previous input.  The drift step, the Foellmer score
  correction and the noise amplitude fold into the four host scalars of ``step_coefficients`` (fp64, rounded once); the step times
  are the host's own ``linspace``, so nothing is read back from the device.  One further launch writes the first input from x0,
  and the last step writes ``x_new`` alone.  Every step writes a fresh tensor: nothing a network backward has saved is overwritten.

With the Foellmer choice (steps i >= 1; g^2 = |2 sigma^2 s d beta / beta - 2 s sigma d sigma - sigma^2| = eps^2 (1 - s)(3 - s)):
    k = (g^2 - sigma^2) A / 2 = 1 / (s^2 (2 - s)),  A = 1 / (s sigma (d beta sigma - beta d sigma))
    bhat = b + k (beta b - d beta x - (beta d alpha - d beta alpha) x0)
    cx = 1 - 2 D / (s (2 - s)),  cb = D (3 - s) / (2 - s),  c0 = D / s,  cn = eps sqrt((1 - s)(3 - s) D)          (D = delta s)
and without it cx = 1, cb = D, c0 = 0, cn = sigma(s) sqrt(D).

Stated deviations from the reference:

* the sampler broadcasts the ``(1, St, H, W)`` static planes over the batch; the reference's ``cat`` in ``_forward_eval`` only
  works for ``B = 1`` when static features are present.
* ``input_dtype=torch.bfloat16`` writes the network input (and with it the sampler's carried state) in bf16; the reference's type
  promotion always gives float32, and ``None`` reproduces that.  Drift target and sampler result are float32.
* CPU tensors raise: the HIP path has no CPU fallback.
* history (``n_history > 0``) raises, as in the reference.
* the noise module keeps its generator as a device counter (``makani_amd.noise``), so ``get_internal_rng`` returns the wrapper's own
  ``torch.Generator`` — the one the ``s`` draw uses — instead of the noise module's.
* on a sphere split over h x w ranks the generator of ``s`` is seeded WITHOUT the model-rank term, and the noise with
  ``noise_seed_reflect(..., share_over_model=True)``: ranks that hold shards of one sample must draw the same ``s`` and hold shards
  of one noise field.  The reference's offset includes the model rank.
* ``forward(..., s=, noise=)`` are keyword-only test hooks: ``s`` (B, S) replaces the uniform draw (before the antithetic
  mirror); ``noise`` replaces the noise module's draws, either as fields ``(K, B, C, H, W)`` or as innovations of the spectral
  state ``(K, B, 1, C, L, M, 2)`` handed to ``noise_module.update(innovation=)``; K = 1 in training, ``n_steps`` in sampling.
"""
import math

import torch
import torch.nn as nn

from . import _lib, comm
from .ops import SiStepFn, si_assemble


def step_coefficients(s, ds, eps, foellmer=False, first=False):
    """``(cx, cb, c0, cn)`` of ``x <- cx x + cb b + c0 x0 + cn z`` for the step at time ``s`` of width ``ds``, in fp64 python
    floats.  The first step of the sampler (``first``) is the plain Euler-Maruyama step whatever ``foellmer`` says."""
    s, ds, eps = float(s), float(ds), float(eps)
    if first or not foellmer:
        return 1.0, ds, 0.0, eps * (1.0 - s) * math.sqrt(ds)
    if not 0.0 < s < 1.0:
        raise ValueError(f"the Foellmer correction is singular at s = {s}: it is evaluated strictly inside (0, 1)")
    return (1.0 - 2.0 * ds / (s * (2.0 - s)), ds * (3.0 - s) / (2.0 - s), ds / s, eps * math.sqrt((1.0 - s) * (3.0 - s) * ds))


class InterpolationWrapper(nn.Module):
    """``model(cat([x0, x, xu, static, s plane]))``: the network sees the time as one more input plane"""

    def __init__(self, model_handle, n_pred_chans, n_static_channels, n_dynamic_channels):
        super().__init__()
        inp_chans = n_pred_chans * 2 + n_static_channels + n_dynamic_channels + 1
        self.model = model_handle(inp_chans=inp_chans)

    def forward(self, x0, x, xu, static, s):
        s = s.reshape(s.shape[0], 1, 1, 1)
        s = torch.tile(s, (1, 1, x.shape[-2], x.shape[-1]))
        parts = [x0, x] + [t for t in (xu, static) if t is not None] + [s]
        return self.model(torch.cat(parts, dim=-3))


class TimeAwareInterpolationWrapper(nn.Module):
    """``model(cat([x0, x, xu, static]), s[:, None])``: the network takes the time as a second argument"""

    def __init__(self, model_handle, n_pred_chans, n_static_channels, n_dynamic_channels):
        super().__init__()
        inp_chans = n_pred_chans * 2 + n_static_channels + n_dynamic_channels
        self.model = model_handle(inp_chans=inp_chans)

    def forward(self, x0, x, xu, static, s):
        parts = [x0, x] + [t for t in (xu, static) if t is not None]
        return self.model(torch.cat(parts, dim=-3), s.unsqueeze(1))


def _seed_offset(share_over_model=False):
    """the reference's per-rank offset (stochastic_interpolant.py:215-219); ``share_over_model``: the model rank enters as 0"""
    nmodel = comm.get_size("model")
    rank_m = 0 if share_over_model else comm.get_rank("model")
    return rank_m + nmodel * comm.get_rank("batch") + nmodel * comm.get_size("batch") * comm.get_rank("ensemble")


class StochasticInterpolantWrapper(nn.Module):
    """See the module docstring.  ``StochasticInterpolantWrapper(model, preprocessor, noise_module, *, n_pred_chans,
    noise_epsilon=1.0, use_foellmer=False, antithetic_sampling=False, time_aware=False, seed=333, input_dtype=None,
    share_over_model=None)``.  ``model`` is an ``InterpolationWrapper`` / ``TimeAwareInterpolationWrapper`` (a bare network is
    wrapped), ``preprocessor`` a ``Preprocessor2D`` without history, ``noise_module`` an ``IsotropicGaussianRandomFieldS2`` with
    ``n_pred_chans`` channels and one time level.  ``share_over_model``: seed the generator of ``s`` without the model-rank term
    (``None``: whenever the spatial group has more than one rank, which is what ``from_params`` passes)."""

    def __init__(self, model, preprocessor, noise_module, *, n_pred_chans, noise_epsilon=1.0, use_foellmer=False,
                 antithetic_sampling=False, time_aware=False, seed=333, input_dtype=None, share_over_model=None):
        super().__init__()
        if getattr(preprocessor, "n_history", 0) != 0:
            raise ValueError(f"this model currently does not support history, expected n_history == 0 but got {preprocessor.n_history}")
        if input_dtype not in (None, torch.float32, torch.bfloat16):
            raise TypeError(f"input_dtype is None, torch.float32 or torch.bfloat16, not {input_dtype}")
        want = TimeAwareInterpolationWrapper if time_aware else InterpolationWrapper
        if isinstance(model, (InterpolationWrapper, TimeAwareInterpolationWrapper)):
            if not isinstance(model, want):
                raise TypeError(f"time_aware = {time_aware} needs a {want.__name__}, got a {type(model).__name__}")
        else:
            model = want(lambda inp_chans: model, n_pred_chans, 0, 0)
        self.preprocessor = preprocessor
        self.model = model
        self.noise_module = noise_module
        self.n_pred_chans = int(n_pred_chans)
        self.time_aware = bool(time_aware)
        self.use_foellmer = use_foellmer
        self.antithetic_sampling = antithetic_sampling
        self.noise_epsilon = noise_epsilon
        self.input_dtype = input_dtype
        if share_over_model is None:
            share_over_model = comm.get_size("spatial") > 1
        self._rng_seed = seed + 333 + _seed_offset(share_over_model)
        self.rng_cpu = torch.Generator(device=torch.device("cpu"))
        self.rng_cpu.manual_seed(self._rng_seed)
        self._rng_gpu = None
        # the schedule as tensor functions, for gsq_fn / dlog_rho / stochastic_path
        self.alpha_fn = lambda s: 1.0 - s
        self.dalpha_fn = lambda s: -1.0
        self.beta_fn = lambda s: torch.square(s)
        self.dbeta_fn = lambda s: 2.0 * s
        self.sigma_fn = lambda s: self.noise_epsilon * (1.0 - s)
        self.dsigma_fn = lambda s: -1.0 * self.noise_epsilon
        self.gamma_fn = lambda s: torch.sqrt(s) * self.sigma_fn(s)
        self.dgamma_fn = lambda s: torch.sqrt(s) * self.dsigma_fn(s)

    @classmethod
    def from_params(cls, params, model_handle, noise_epsilon=1.0, use_foellmer=False, antithetic_sampling=False, seed=333,
                    input_dtype=None, static_features=None, **kwargs):
        """What ``StochasticInterpolantWrapper(params, model_handle, ...)`` of the reference builds: ``Preprocessor2D.from_params``,
        the isotropic Gaussian field on ``(img_crop_shape_x, img_crop_shape_y)`` / ``data_grid_type`` (sigma = 1, alpha = 0, one
        time level, ``batch_size`` entries, ``N_in_predicted_channels`` channels) and ``model_handle(inp_chans=...)`` behind the
        plain or the time-aware wrapper (``params.time_aware``).  ``static_features`` goes to ``Preprocessor2D.from_params``."""
        from .noise import IsotropicGaussianRandomFieldS2, noise_seed_reflect
        from .preprocessor import Preprocessor2D
        get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
        if params.n_history != 0:
            raise ValueError(f"this model currently does not support history, expected n_history == 0 but got {params.n_history}")
        if params.n_future != 0:
            raise ValueError(f"this model currently does not support future steps, expected n_future == 0 but got {params.n_future}")
        preprocessor = Preprocessor2D.from_params(params, static_features=static_features)
        n_pred_chans = params.N_in_predicted_channels
        if n_pred_chans != params.N_out_channels:
            raise ValueError(f"expected N_in_predicted_channels ({n_pred_chans}) to match N_out_channels ({params.N_out_channels})")
        time_aware = bool(get("time_aware", False))
        wrapper = TimeAwareInterpolationWrapper if time_aware else InterpolationWrapper
        model = wrapper(model_handle, n_pred_chans, params.N_static_channels, params.N_dynamic_channels)
        split = comm.get_size("spatial") > 1
        if split:
            noise_seed, _ = noise_seed_reflect(False, seed_offset=seed - 333, share_over_model=True)
        else:
            noise_seed = seed + _seed_offset()
        noise = IsotropicGaussianRandomFieldS2((params.img_crop_shape_x, params.img_crop_shape_y), params.batch_size, n_pred_chans,
                                               num_time_steps=1, sigma=1.0, alpha=0.0, grid_type=params.data_grid_type, seed=noise_seed)
        return cls(model, preprocessor, noise, n_pred_chans=n_pred_chans, noise_epsilon=noise_epsilon, use_foellmer=use_foellmer,
                   antithetic_sampling=antithetic_sampling, time_aware=time_aware, seed=seed, input_dtype=input_dtype,
                   share_over_model=split)

    # ---- generators ---------------------------------------------------------------------------------------------
    @property
    def rng_gpu(self):
        """the device generator of the ``s`` draw, created on the current GPU at its first use"""
        if self._rng_gpu is None:
            self._rng_gpu = torch.Generator(device=torch.device("cuda", torch.cuda.current_device()))
            self._rng_gpu.manual_seed(self._rng_seed)
        return self._rng_gpu

    def get_internal_rng(self, gpu=True):
        return self.rng_gpu if gpu else self.rng_cpu

    # ---- the schedule as tensor functions (not the hot path) ----------------------------------------------------------
    def gsq_fn(self, s, foellmer=False):
        """g^2(s): sigma^2, or the Foellmer process's diffusion |2 sigma^2 s d beta / beta - 2 s sigma d sigma - sigma^2|"""
        sig = self.sigma_fn(s)
        if not foellmer:
            return torch.square(sig)
        ratio = torch.where(s > 0, s * self.dbeta_fn(s) / self.beta_fn(s), 2.0)
        return torch.abs(2.0 * torch.square(sig) * ratio - 2.0 * s * sig * self.dsigma_fn(s) - torch.square(sig))

    def dlog_rho(self, x, x0, b, s):
        """the score of the interpolant density from the drift ``b``; singular at s = 0 and s = 1"""
        sig, beta, dbeta = self.sigma_fn(s), self.beta_fn(s), self.dbeta_fn(s)
        As = 1.0 / (s * sig * (dbeta * sig - beta * self.dsigma_fn(s)))
        cs = x * dbeta + (beta * self.dalpha_fn(s) - dbeta * self.alpha_fn(s)) * x0
        return As * (beta * b - cs)

    def stochastic_path(self, x0, x1, noise, s, return_derivative=True):
        """interpolant (and drift) of x0, x1, noise (B, S, ...) at the times s (B, S)"""
        sr = s.reshape(s.shape[0], s.shape[1], *[1] * (x0.dim() - 2))
        interp = self.alpha_fn(sr) * x0 + self.beta_fn(sr) * x1 + self.gamma_fn(sr) * noise
        if not return_derivative:
            return interp
        return interp, self.dalpha_fn(sr) * x0 + self.dbeta_fn(sr) * x1 + self.dgamma_fn(sr) * noise

    # ---- the two modes ----------------------------------------------------------------------------------------------
    def _features(self, B):
        """xu (B, U, H, W) | None and static (St, H, W) | None, read in place from the preprocessor"""
        xu = self.preprocessor._unpredicted(False)
        if xu is not None:
            if xu.shape[0] != B:
                raise RuntimeError(f"batch mismatch between input ({B}) and cached unpredicted features ({xu.shape[0]})")
            xu = xu.detach().squeeze(1)
        static = self.preprocessor._static()
        return xu, (None if static is None else static.detach())

    def _draws(self, noise, count):
        """the ``count`` noise fields (B, C, H, W) of one call, in order: the module's own, or the injected ones"""
        if noise is not None:
            noise = torch.as_tensor(noise)
            if noise.shape[0] != count:
                raise ValueError(f"noise: expected {count} draws along the first dimension, got {noise.shape[0]}")
        for k in range(count):
            with torch.no_grad():
                if noise is None:
                    z = self.noise_module(update_internal_state=True).squeeze(1)
                elif noise.dim() == 7:
                    self.noise_module.update(innovation=noise[k])
                    z = self.noise_module().squeeze(1)
                else:
                    z = noise[k]
            yield z

    def _net(self, x_in, s):
        if self.time_aware:
            return self.model.model(x_in, s.unsqueeze(1))
        return self.model.model(x_in)

    def _x0(self, inp):
        _lib.need_gpu(inp, "interpolant")
        if inp.dim() != 4:
            raise RuntimeError(f"expected a 4D input, got {inp.dim()}D")
        if inp.shape[1] != self.n_pred_chans:
            raise RuntimeError(f"the input has {inp.shape[1]} channels, the interpolant {self.n_pred_chans}")
        return _lib.prep(inp)

    def _out_dtype(self):
        return torch.float32 if self.input_dtype is None else self.input_dtype

    def _forward_train(self, inp, tar, n_samples=1, s=None, noise=None):
        x0 = self._x0(inp)
        B = x0.shape[0]
        with torch.no_grad():
            xu, static = self._features(B)
            if s is None:
                s = torch.empty((B, n_samples), dtype=torch.float32, device=x0.device)
                s.uniform_(0.0, 1.0, generator=self.rng_gpu)
            else:
                s = torch.as_tensor(s, dtype=torch.float32, device=x0.device).reshape(B, -1)
            if self.antithetic_sampling:
                s = torch.cat([s, 1.0 - s], dim=1)
            (z,) = self._draws(noise, 1)
            x_in, drift = si_assemble(x0.detach(), tar.detach(), z, s, xu, static, self.noise_epsilon, has_s=not self.time_aware,
                                      out_dtype=self._out_dtype())
        return self._net(x_in, s.flatten()), drift

    def _forward_eval(self, inp, n_steps=1, noise=None):
        x0 = self._x0(inp)
        B, C = x0.shape[0], self.n_pred_chans
        if n_steps < 1:
            raise ValueError(f"n_steps = {n_steps} must be positive")
        xu, static = self._features(B)
        # the reference's own float32 linspace and its differences, known to the host
        stens = torch.linspace(0, 1, n_steps + 1, dtype=torch.float32)
        delta = (stens[1:] - stens[:-1]).double().tolist()
        stens = stens.double().tolist()
        has_s, odt = not self.time_aware, self._out_dtype()

        def svec(v):
            return torch.full((B,), v, dtype=torch.float32, device=x0.device) if self.time_aware else None

        draws = self._draws(noise, n_steps)
        x_in = SiStepFn.apply(x0, None, x0, None, xu, static, (1.0, 0.0, 0.0, 0.0), stens[0], False, has_s, odt)
        for i in range(n_steps):
            b = self._net(x_in, svec(stens[i]))
            z = next(draws)
            coef = step_coefficients(stens[i], delta[i], self.noise_epsilon, foellmer=self.use_foellmer, first=i == 0)
            last = i == n_steps - 1
            x = x0 if i == 0 else x_in[:, C:2 * C]
            x_in = SiStepFn.apply(x, b, x0, z, xu, static, coef, stens[i + 1], last, has_s, torch.float32 if last else odt)
        return x_in

    @_lib.device_guard
    def forward(self, inp, tar=None, n_samples=1, n_steps=1, *, s=None, noise=None):
        """Training mode: ``(drift_pred, drift)``, both (B S', C, H, W), for ``n_samples`` interpolant times per batch entry
        (twice as many rows with antithetic sampling).  Evaluation mode: the forecast (B, C, H, W) of an ``n_steps`` SDE sampler."""
        _lib.need_gpu(inp, "interpolant")
        self.preprocessor.update_internal_state(replace_state=True, batch_size=inp.shape[0])
        self.noise_module.update(replace_state=True, batch_size=inp.shape[0])
        if self.training:
            if tar is None:
                raise ValueError("training mode needs the target tar")
            return self._forward_train(inp, tar, n_samples=n_samples, s=s, noise=noise)
        return self._forward_eval(inp, n_steps=n_steps, noise=noise)
