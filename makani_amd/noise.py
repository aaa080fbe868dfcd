"""Input-noise processes on the sphere behind the interface of ``makani/models/noise.py``: ``BaseNoiseS2``,
``IsotropicGaussianRandomFieldS2`` ("white"), ``DiffusionNoiseS2`` ("diffusion"), ``DummyNoiseS2`` ("dummy"), ``build_noise``
and ``noise_seed_reflect``; ``InputNoise`` restates what ``Preprocessor2D`` does with them (``preprocessor.py:434-455,872-928``).

Constructor arguments, attributes, buffers (``state``, ``sigma_l``, ``phi``, ``discount``: non-persistent, the reference's
shapes and values) and the state layout ``(B, T, C, L, M, 2)`` are the reference's, so ``get/set_tensor_state`` interchange
with it.  What differs:

* ``update`` is ONE HIP kernel over the state, in place (``csrc/noise.hip``): it draws the innovations (Philox4x32-10,
  Box-Muller) and applies the white / autoregressive / replace rule in the same pass, followed by a one-thread kernel that
  advances the counter.  Both only touch device memory, so ``update(); forward()`` can be captured in a hipGraph and each
  replay draws the next innovations.  ``update(..., innovation=xi)`` uses the given innovations instead (the counter stays).
* the generator is a non-persistent ``int64[2]`` buffer ``rng = {seed, offset}`` instead of two ``torch.Generator``s:
  ``get_rng_state()`` returns ``(None, rng.cpu().clone())`` and ``set_rng_state(cpu_state, gpu_state)`` restores from
  ``gpu_state``.  The stream of normals is this package's own, not torch's.
* ``forward`` is the package's ``InverseRealSHT`` on ``view_as_complex(state)`` (no copy).
* on a sphere split over h x w ranks (``comm.get_size("spatial") > 1`` with the ``h`` / ``w`` groups behind it) the spectral
  state is split over h (degree l) and w (order m) as in the reference and ``forward`` is ``DistributedInverseRealSHT``, but the
  counter of every element is its GLOBAL index (``mk_noise_update_shard``): ranks that share a seed
  (``noise_seed_reflect(..., share_over_model=True)``) hold exactly the slices of the serial state, whatever the layout.
  A spatial group without h / w groups behind it raises ``NotImplementedError`` ("serial only").
* construction and the buffer mathematics work on the CPU; ``update`` / ``forward`` need the module on a GPU.
"""
import math

import torch
import torch.nn as nn

from . import _lib, comm
from .sht import InverseRealSHT

MODE_WHITE, MODE_AR, MODE_REPLACE = (_lib.CONSTS["MK_NOISE_" + k] for k in ("WHITE", "AR", "REPLACE"))


class BaseNoiseS2(nn.Module):
    """Common machinery: the inverse SHT, the counter of the generator and the spectral ``state`` buffer
    ``(B, T, C, lmax, mmax, 2)``.  ``update`` of the base class overwrites the state with fresh standard normals."""

    def __init__(self, img_shape, batch_size, num_channels, num_time_steps, grid_type="equiangular", lmax=None, seed=333,
                 reflect=False, **kwargs):
        super().__init__()
        self.nlat, self.nlon = img_shape
        self.num_channels = num_channels
        self.num_time_steps = num_time_steps
        self.reflect = reflect
        self.spatial_parallel = comm.get_size("spatial") > 1
        if self.spatial_parallel:
            from . import distributed as thd
            if comm.get_size("h") * comm.get_size("w") != comm.get_size("spatial") or not thd.ensure_initialized():
                raise NotImplementedError("noise on a spatially split sphere needs the h / w groups of the distributed inverse SHT "
                                          "behind the spatial group: without them the HIP noise processes are serial only")
            self.isht = isht = thd.DistributedInverseRealSHT(self.nlat, self.nlon, lmax=lmax, mmax=lmax, grid=grid_type)
            ih, iw = isht.comm_rank_polar, isht.comm_rank_azimuth
            self.lmax_local, self.mmax_local = isht.l_shapes[ih], isht.m_shapes[iw]
            self.nlat_local, self.nlon_local = isht.lat_shapes[ih], isht.lon_shapes[iw]
            self.l_off, self.m_off = isht.l_off, isht.m_off
            self.lat_off, self.lon_off = sum(isht.lat_shapes[:ih]), sum(isht.lon_shapes[:iw])
        else:
            self.isht = InverseRealSHT(self.nlat, self.nlon, lmax=lmax, mmax=lmax, grid=grid_type)
            self.lmax_local, self.mmax_local = self.isht.lmax, self.isht.mmax
            self.nlat_local, self.nlon_local = self.nlat, self.nlon
            self.l_off = self.m_off = self.lat_off = self.lon_off = 0
        self.lmax, self.mmax = self.isht.lmax, self.isht.mmax
        self.set_rng(seed=seed)
        self._ensure_state(batch_size, device=torch.device("cpu"), dtype=torch.float32)

    # ---- state --------------------------------------------------------------------------------------------------
    @property
    def _state_shape_suffix(self):
        """shape of ``state`` behind the batch dimension"""
        return (self.num_time_steps, self.num_channels, self.lmax_local, self.mmax_local, 2)

    def _ensure_state(self, batch_size, device=None, dtype=None):
        """(re-)register ``state`` as zeros of the wanted batch size; nothing happens when the shape already fits"""
        have = "state" in self._buffers
        if device is None:
            device = self.state.device if have else torch.device("cpu")
        if dtype is None:
            dtype = self.state.dtype if have else torch.float32
        shape = (batch_size, *self._state_shape_suffix)
        if not have or tuple(self.state.shape) != shape:
            self.register_buffer("state", torch.zeros(shape, dtype=dtype, device=device), persistent=False)

    def is_stateful(self):
        raise NotImplementedError("is_stateful method not implemented for this noise class")

    def extra_repr(self):
        return (f"img_shape=({self.nlat}, {self.nlon}), num_channels={self.num_channels}, "
                f"num_time_steps={self.num_time_steps}, lmax={self.lmax}, reflect={self.reflect}")

    def reset(self, batch_size=None):
        if batch_size is not None:
            self._ensure_state(batch_size)
        with torch.no_grad():
            self.state.zero_()

    def get_tensor_state(self):
        return self.state.detach().clone()

    def set_tensor_state(self, newstate):
        want = tuple(self._state_shape_suffix)
        got = tuple(newstate.shape[1:]) if newstate.dim() >= 1 else tuple(newstate.shape)
        if got != want:
            raise ValueError(f"set_tensor_state: shape mismatch beyond batch dim. Expected suffix {want}, got {got} "
                             f"(full newstate.shape={tuple(newstate.shape)}, current state.shape={tuple(self.state.shape)}).")
        if tuple(newstate.shape) != tuple(self.state.shape):
            self._ensure_state(newstate.shape[0])
        with torch.no_grad():
            self.state.copy_(newstate)

    # ---- generator ----------------------------------------------------------------------------------------------
    def set_rng(self, seed=333):
        """``rng = {seed, 0}``: the key of the generator and the number of time levels drawn so far"""
        value = torch.tensor([int(seed), 0], dtype=torch.int64)
        if "rng" in self._buffers:
            self.rng.copy_(value)
        else:
            self.register_buffer("rng", value, persistent=False)

    def get_rng_state(self):
        return None, self.rng.cpu().clone()

    def set_rng_state(self, cpu_state, gpu_state):
        if gpu_state is not None:
            self.rng.copy_(torch.as_tensor(gpu_state, dtype=torch.int64).reshape(2))

    # ---- update -------------------------------------------------------------------------------------------------
    def _kernel_box(self):
        """(R, S, r0, Rl, s0, Sl): one (batch entry, channel) plane of the GLOBAL time level as the kernel counts it, R rows of
        S floats in the reference's memory order, and this rank's rows [r0, r0 + Rl) and floats [s0, s0 + Sl) of it"""
        return self.lmax, 2 * self.mmax, self.l_off, self.lmax_local, 2 * self.m_off, 2 * self.mmax_local

    def _launch(self, mode, innovation=None, sigma=None, phi=None):
        """one pass over ``state`` (mk_noise_update, on a split sphere mk_noise_update_shard), then the counter moves on by the
        time levels drawn"""
        self._require_gpu()
        state = self.state
        if state.dtype != torch.float32 or not state.is_contiguous():
            raise TypeError(f"the noise state has to be contiguous float32, got {state.dtype}")
        B, T, C = state.shape[0], self.num_time_steps, self.num_channels
        R, S, r0, Rl, s0, Sl = self._kernel_box()
        levels = 1 if mode == MODE_AR else T
        xi = None
        if innovation is not None:
            want = (B, levels, *state.shape[2:])
            if tuple(innovation.shape) != want:
                raise ValueError(f"innovation: expected shape {want}, got {tuple(innovation.shape)}")
            xi = innovation.detach().to(device=state.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(state.device):
            L_ = _lib.lib()
            args = (_lib.ptr(state), _lib.ptr(xi), _lib.ptr(sigma), _lib.ptr(phi), _lib.ptr(self.rng), mode, B, T, C)
            if self.spatial_parallel:
                _lib.check(L_.mk_noise_update_shard(*args, R, S, r0, Rl, s0, Sl, int(bool(self.reflect)), _lib.stream()),
                           "mk_noise_update_shard")
            else:
                _lib.check(L_.mk_noise_update(*args, R, S // 2, int(bool(self.reflect)), _lib.stream()), "mk_noise_update")
            if xi is None:
                _lib.check(L_.mk_noise_advance(_lib.ptr(self.rng), levels, _lib.stream()), "mk_noise_advance")

    def update(self, replace_state=False, batch_size=None, innovation=None):
        """state = fresh standard normals (negated with ``reflect``); ``replace_state`` has no meaning here"""
        if batch_size is not None:
            self._ensure_state(batch_size)
        with torch.no_grad():
            self._launch(MODE_WHITE, innovation)

    def _field(self, cstate):
        """(B, T, C, L, M) complex64 -> (B, T, C, nlat, nlon) on the grid"""
        B = cstate.shape[0]
        cstate = cstate.reshape(B, self.num_time_steps * self.num_channels, self.lmax_local, self.mmax_local)
        with torch.autocast(device_type=cstate.device.type, enabled=False):
            eta = self.isht(cstate)
        return eta.reshape(B, self.num_time_steps, self.num_channels, self.nlat_local, self.nlon_local)

    def _require_gpu(self):
        if not self.state.is_cuda:
            raise RuntimeError("makani_amd noise processes need the module on a GPU (the HIP path has no CPU fallback)")


class IsotropicGaussianRandomFieldS2(BaseNoiseS2):
    """Stateless isotropic Gaussian field with the power-law spectrum ``sigma_l ~ (2l + 1)^(-alpha / 2)``, normalised to the
    pointwise variance ``sigma^2`` (Lang & Schwab 2015).  ``sigma_l`` (1, 1, 1, L, M), zero for m > l, is applied in
    ``forward`` with torch operations: with ``learnable=True`` it is a parameter and autograd gives its gradient.  On a split
    sphere ``sigma_l`` is this rank's (l, m) slice."""

    def __init__(self, img_shape, batch_size, num_channels, num_time_steps=1, sigma=1.0, alpha=0.0, grid_type="equiangular",
                 lmax=None, seed=333, reflect=False, learnable=False, **kwargs):
        super().__init__(img_shape=img_shape, batch_size=batch_size, num_channels=num_channels, num_time_steps=num_time_steps,
                         grid_type=grid_type, lmax=lmax, seed=seed, reflect=reflect)
        self.sigma, self.alpha, self.learnable = sigma, alpha, learnable
        degree = torch.arange(self.lmax).reshape(-1, 1)
        order = torch.arange(self.mmax)
        spectrum = torch.pow(2 * degree + 1, -float(alpha))
        norm = torch.sum((2 * degree + 1) * spectrum / 4.0 / math.pi)
        sigma_l = torch.where(order <= degree, sigma * torch.sqrt(spectrum / norm), 0.0)
        sigma_l = sigma_l.reshape(1, 1, 1, self.lmax, self.mmax).to(dtype=torch.float32)
        sigma_l = sigma_l[..., self.l_off:self.l_off + self.lmax_local, self.m_off:self.m_off + self.mmax_local].contiguous()
        if learnable:
            self.register_parameter("sigma_l", nn.Parameter(sigma_l))
            self.sigma_l.sharded_dims_mp = [None, None, None, "h", "w"]
        else:
            self.register_buffer("sigma_l", sigma_l, persistent=False)

    def is_stateful(self):
        return False

    def extra_repr(self):
        return super().extra_repr() + f", sigma={self.sigma}, alpha={self.alpha}, learnable={self.learnable}"

    @torch.compiler.disable
    def forward(self, update_internal_state=False):
        self._require_gpu()
        eta = self._field(torch.view_as_complex(self.state / math.sqrt(2)) * self.sigma_l)
        if update_internal_state:
            self.update()
        return eta


class DiffusionNoiseS2(BaseNoiseS2):
    """Stateful Ornstein-Uhlenbeck process per spherical-harmonic coefficient (Palmer et al. 2009, appendix 8.1):
    ``eta <- phi eta + sigma_l xi`` with ``phi = exp(-lambd)`` and ``sigma_l`` carrying ``sqrt(1 - phi^2)`` and the heat-kernel
    spectrum ``exp(-kT l (l + 1) / 2)``; ``kT`` and ``lambd`` scalar or one value per channel.  ``update(replace_state=True)``
    draws the whole history of ``num_time_steps`` levels from the stationary distribution."""

    def __init__(self, img_shape, batch_size, num_channels, num_time_steps=1, sigma=1.0, kT=0.5 * (500.0 / 6370.0) ** 2,
                 lambd=1.0, grid_type="equiangular", lmax=None, seed=333, reflect=False, learnable=False, **kwargs):
        super().__init__(img_shape=img_shape, batch_size=batch_size, num_channels=num_channels, num_time_steps=num_time_steps,
                         grid_type=grid_type, lmax=lmax, seed=seed, reflect=reflect)
        self.sigma, self.kT, self.lambd, self.learnable = sigma, kT, lambd, learnable
        C = num_channels

        def per_channel(value, name):
            if isinstance(value, list):
                value = torch.as_tensor(value)
                if value.dim() != 1:
                    raise ValueError(f"expected {name} to be a 1D tensor, got shape {tuple(value.shape)}")
                if value.shape[0] != C:
                    raise ValueError(f"expected {name} to have {C} entries (one per channel), got {value.shape[0]}")
            else:
                value = torch.as_tensor([value]).repeat(C)
            return value.reshape(C, 1)

        kT, lambd = per_channel(kT, "kT"), per_channel(lambd, "lambd")
        degree = torch.arange(self.lmax)
        heat = torch.exp(-kT * degree * (degree + 1))
        norm = torch.sum((2 * degree[1:] + 1) * heat[..., 1:], dim=-1, keepdim=True)
        phi = torch.exp(-lambd)
        amp = sigma * torch.sqrt(0.5 * (1 - phi**2) / norm)
        sigma_l = math.sqrt(4 * math.pi) * (amp * torch.exp(-0.5 * kT * degree * (degree + 1)))
        phi = phi.reshape(C, 1, 1, 1).to(dtype=torch.float32)                          # (C, L, M, 2) broadcast
        sigma_l = sigma_l.reshape(1, 1, C, self.lmax, 1, 1).to(dtype=torch.float32)    # (B, T, C, L, M, 2) broadcast
        sigma_l = sigma_l[:, :, :, self.l_off:self.l_off + self.lmax_local].contiguous()     # this rank's degrees
        if learnable:
            self.phi = nn.Parameter(phi)
            self.phi.is_shared_mp = ["matmul", "h", "w"]
            self.phi.sharded_dims_mp = [None, None, None]
            self.sigma_l = nn.Parameter(sigma_l)
            self.sigma_l.is_shared_mp = ["matmul", "w"]
            self.sigma_l.sharded_dims_mp = [None, None, None, "h", None, None]
        else:
            self.register_buffer("phi", phi, persistent=False)
            self.register_buffer("sigma_l", sigma_l, persistent=False)
        if self.num_time_steps > 1:
            if learnable:
                raise NotImplementedError("num_time_steps>1 learnable diffusion noise not supported")
            # discount[c][t][r] = phi_c^(t - r) for r <= t: the history of a replace draw (the kernel runs the recurrence)
            lag = torch.arange(self.num_time_steps).reshape(-1, 1) - torch.arange(self.num_time_steps)
            power = torch.pow(self.phi.reshape(C, 1, 1).to(torch.float64), lag.clamp(min=0).to(torch.float64))
            discount = torch.where(lag >= 0, power, 0.0).to(dtype=torch.float32)
            self.register_buffer("discount", discount, persistent=False)

    def is_stateful(self):
        return True

    def extra_repr(self):
        return super().extra_repr() + f", sigma={self.sigma}, kT={self.kT}, lambd={self.lambd}, learnable={self.learnable}"

    def update(self, replace_state=False, batch_size=None, innovation=None):
        """one autoregressive step (the oldest level drops out), or with ``replace_state`` a fresh stationary history"""
        if batch_size is not None:
            self._ensure_state(batch_size)
        with torch.no_grad():
            sigma = self.sigma_l.detach().reshape(self.num_channels, self.lmax_local)
            phi = self.phi.detach().reshape(self.num_channels)
            self._launch(MODE_REPLACE if replace_state else MODE_AR, innovation, sigma, phi)

    @torch.compiler.disable
    def forward(self, update_internal_state=False):
        self._require_gpu()
        eta = self._field(torch.view_as_complex(self.state))
        if update_internal_state:
            self.update()
        return eta


class DummyNoiseS2(BaseNoiseS2):
    """Noise of the right shape without a transform, for tests of shapes and control flow: the state lives on the grid,
    ``(B, T, C, nlat, nlon)``, and ``forward`` returns it (the live buffer, as the reference does).  ``constant_zero`` keeps
    zeros, ``constant_random`` redraws standard normals with every ``update``.  On a split sphere the state is the rank's
    latitude / longitude slice of the serial one."""

    def __init__(self, img_shape, batch_size, num_channels, num_time_steps=1, mode="constant_zero", seed=333, **kwargs):
        if mode not in ("constant_zero", "constant_random"):
            raise ValueError(f"DummyNoiseS2: unknown mode '{mode}'. Expected 'constant_zero' or 'constant_random'.")
        self.mode = mode
        super().__init__(img_shape=img_shape, batch_size=batch_size, num_channels=num_channels, num_time_steps=num_time_steps,
                         seed=seed)

    @property
    def _state_shape_suffix(self):
        return (self.num_time_steps, self.num_channels, self.nlat_local, self.nlon_local)

    def _kernel_box(self):
        if self.nlon % 2:
            raise NotImplementedError("DummyNoiseS2 'constant_random' needs an even number of longitudes")
        return self.nlat, self.nlon, self.lat_off, self.nlat_local, self.lon_off, self.nlon_local

    def is_stateful(self):
        return False

    def extra_repr(self):
        return super().extra_repr() + f", mode={self.mode}"

    def update(self, replace_state=False, batch_size=None, innovation=None):
        if batch_size is not None:
            self._ensure_state(batch_size)
        self._require_gpu()
        with torch.no_grad():
            if self.mode == "constant_zero":
                self.state.zero_()
            else:
                self._launch(MODE_WHITE, innovation)

    def forward(self, update_internal_state=False):
        self._require_gpu()
        state = self.state
        if update_internal_state:
            self.update()
        return state


def noise_seed_reflect(centered: bool, seed_offset: int = 0, *, share_over_model: bool = False):
    """Per-rank base seed and reflection flag of a noise source.  Not centered: every (model rank, data rank) has its own
    seed.  Centered: the ensemble ranks (0, 1), (2, 3), ... share a seed and differ by the sign of every draw.
    ``share_over_model``: the model rank enters as 0, so the h x w ranks of one model instance share a stream and, the counter
    being global, hold the shards of ONE field — the serial one; the default is the reference's seed per model rank."""
    nmodel = comm.get_size("model")
    rank_m = 0 if share_over_model else comm.get_rank("model")
    if not centered:
        return 333 + seed_offset + rank_m + nmodel * comm.get_rank("data"), False
    rank_e = comm.get_rank("ensemble")
    seed = 333 + seed_offset + rank_m + nmodel * (rank_e // 2) + nmodel * comm.get_size("ensemble") * comm.get_rank("batch")
    return seed, rank_e % 2 == 0


def build_noise(noise_params, *, img_shape, batch_size, num_channels, num_time_steps, grid_type, seed, reflect, default_lambd=1.0):
    """The noise module a config dict asks for (``type``: "diffusion" | "white" | "dummy")."""
    kind = noise_params.get("type", None)
    if kind is None:
        raise ValueError("Error, please specify a noise type")
    common = dict(img_shape=img_shape, batch_size=batch_size, num_channels=num_channels, num_time_steps=num_time_steps)
    spectral = dict(grid_type=grid_type, lmax=noise_params.get("lmax", None), seed=seed, reflect=reflect,
                    sigma=noise_params.get("sigma", 1.0), learnable=noise_params.get("learnable", False))
    if kind == "diffusion":
        return DiffusionNoiseS2(**common, **spectral, kT=noise_params.get("kT", 0.5 * (100 / 6370) ** 2),
                                lambd=noise_params.get("lambd", default_lambd))
    if kind == "white":
        return IsotropicGaussianRandomFieldS2(**common, **spectral, alpha=noise_params.get("alpha", 0.0))
    if kind == "dummy":
        return DummyNoiseS2(**common)
    raise NotImplementedError(f"Error, noise type {kind} not supported.")


class InputNoise(nn.Module):
    """What ``Preprocessor2D`` does with its ``input_noise`` (``_append_channels`` / ``update_internal_state``):

    * ``forward(x, xc=None)``: ``x`` (B, T, C, H, W) with T = n_history + 1 (or (B, T * C, H, W), returned flattened again).
      "concatenate": the noise channels of every time level go behind ``xc`` (behind ``x`` when there is no ``xc``), and
      ``cat([x, xc], dim=2)`` is returned; "perturb": the noise is added, out of place, to ``perturb_channels`` of ``x``.
    * ``update_internal_state(replace_state, batch_size)`` advances the process and refuses to resize a stateful one in
      the middle of a sequence.
    """

    def __init__(self, noise, mode="concatenate", perturb_channels=None, n_history=0):
        super().__init__()
        if mode not in ("concatenate", "perturb"):
            raise NotImplementedError(f"Error, input noise mode {mode} not supported.")
        if mode == "perturb" and perturb_channels is None:
            raise ValueError("input noise mode 'perturb' needs the list of perturbed channel indices")
        self.input_noise = noise
        self.input_noise_mode = mode
        self.perturb_channels = None if perturb_channels is None else [int(c) for c in perturb_channels]
        self.n_history = int(n_history)

    @classmethod
    def from_params(cls, params, share_over_model=True):
        """The stage ``Preprocessor2D.__init__`` builds from ``params.input_noise`` (``preprocessor.py:149-232``): ``type``,
        ``mode``, ``n_channels`` / ``perturb_channels`` (names looked up in ``params.channel_names``), ``centered``, ``lmax``,
        ``sigma``, ``kT``, ``alpha``, ``learnable``, ``lambd`` (default ``params.dt * params.dhours / 6``); the grid is
        ``(img_shape_x_resampled, img_shape_y_resampled)`` on ``model_grid_type``, the history ``n_history``, the batch
        ``batch_size``.  ``share_over_model``: see ``noise_seed_reflect`` (``False`` gives the reference's seeds)."""
        cfg = params.get("input_noise", None)
        if cfg is None:
            raise ValueError("params.input_noise is not set")
        if "type" not in cfg:
            raise ValueError("Error, please specify an input noise type")
        mode = cfg.get("mode", "concatenate")
        perturb = None
        if mode == "concatenate":
            channels = cfg.get("n_channels", 1)
        elif mode == "perturb":
            perturb = [params.channel_names.index(ch) for ch in cfg.get("perturb_channels", params.channel_names)]
            channels = len(perturb)
        else:
            raise NotImplementedError(f"Error, input noise mode {mode} not supported.")
        seed, reflect = noise_seed_reflect(cfg.get("centered", False), share_over_model=share_over_model)
        lambd = {"default_lambd": params.dt * params.dhours / 6.0} if cfg["type"] == "diffusion" and "lambd" not in cfg else {}
        noise = build_noise(cfg, img_shape=(params.img_shape_x_resampled, params.img_shape_y_resampled),
                            batch_size=params.batch_size, num_channels=channels, num_time_steps=params.n_history + 1,
                            grid_type=params.model_grid_type, seed=seed, reflect=reflect, **lambd)
        return cls(noise, mode=mode, perturb_channels=perturb, n_history=params.n_history)

    def forward(self, x, xc=None):
        flat = x.dim() == 4
        T = self.n_history + 1
        if flat:
            x = x.reshape(x.shape[0], T, x.shape[1] // T, *x.shape[2:])
            if xc is not None:
                xc = xc.reshape(xc.shape[0], T, xc.shape[1] // T, *xc.shape[2:])
        n = self.input_noise()
        if n.shape[0] != x.shape[0]:
            raise RuntimeError(f"batch mismatch between input_noise state ({n.shape[0]}) and input ({x.shape[0]}). Did you call "
                               f"update_internal_state(batch_size=...) at a different batch than the current forward pass?")
        if self.input_noise_mode == "concatenate":
            xc = n if xc is None else torch.cat([xc, n], dim=2)
        else:
            full = torch.zeros_like(x)
            full[:, :, self.perturb_channels] = n
            x = x + full
        out = x if xc is None else torch.cat([x, xc], dim=2)
        return out.flatten(1, 2) if flat else out

    def update_internal_state(self, replace_state=False, batch_size=None):
        current = self.input_noise.state.shape[0]
        if batch_size is not None and not replace_state and current != batch_size and self.input_noise.is_stateful():
            raise RuntimeError(f"update_internal_state: refusing to resize the stochastic noise state from batch {current} to "
                               f"{batch_size} while continuing an autoregressive noise sequence (replace_state={replace_state}): "
                               f"resizing zeroes the n_history+1 time history.  Pass replace_state=True to draw a fresh state "
                               f"at the new batch size, or keep the batch size fixed for the whole rollout.")
        self.input_noise.update(replace_state=replace_state, batch_size=batch_size)
