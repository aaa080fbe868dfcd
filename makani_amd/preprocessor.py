"""``Preprocessor2D`` on the HIP path: what makani's step wrappers run around the network (``makani/models/preprocessor.py``,
``makani/models/stepper.py:76-136,224-315``) — unpredicted / noise channels per time level, quadrature-weighted history
statistics, normalisation of the window, static channels, bias correction and de-normalisation of the prediction.

Per time level the channels are ``[C data | U unpredicted | N noise]``, ``J = C + U + N``, ``T = n_history + 1``.  The kernels
(``csrc/preproc.hip``) read every channel in place from the tensor that holds it — the window ``(B, T·C, H, W)``, the cached
unpredicted features ``(B, T, U, H, W)``, the noise ``(B, T, N, H, W)`` — so the fused path builds no concatenated intermediate:

* ``assemble(inp)`` = ``add_static_features(history_normalize(append_unpredicted_features(inp)))`` after
  ``history_compute_stats``: one statistics launch (plus its tiny merge) and ONE launch that writes the whole network input
  ``(B, T·J + S, H, W)``.  Mode ``"none"`` is the same launch without normalisation and without statistics.
* ``finish(yn)`` = ``history_denormalize(correct_bias(yn), target=True)``: one launch.

The individual methods carry the reference's names, signatures and semantics and run the same kernels with fewer sources, so the
fused result equals their composition bit for bit.  All of them go through autograd functions in which ``history_mean`` and
``history_std`` are differentiable outputs: a rollout without push-forward mode gets the gradient through the statistics
(``dv = g/σ + ω (Gμ + xn Gσ)``, one reduction and one apply launch).  Gradients go to the window and, when it requires grad, to
the noise; unpredicted, static and bias tensors that require grad raise.

Statistics: ``μ = Σ ω v``, ``σ = sqrt(Σ ω (v − μ)²)`` with ``ω[t,h,w] = wt[t] q[h,w]`` (``q`` = ``GridQuadrature(normalize=True)``,
``wt`` = 1/T for ``"mean"``, the normalised ``exp(-decay (n_history − t))`` for ``"exponential"``), fp32, shape ``(B, J, 1, 1)``, no
eps (the reference's ``history_eps`` is unused; a constant channel gives inf / nan as it does there).

With ``spatial_distributed=True`` and a spatial group larger than 1 every rank holds its lat / lon shard of all tensors (static
and bias fields sharded by the caller).  The ranks' ``(Σω, mean, M2)`` in fp64 are all-gathered and merged in rank order on every
rank (identical bits everywhere); backward all-reduces the ``(2, B, J)`` partials of ``Gμ``, ``Gσ``.

Deviations from the reference, each raising ``NotImplementedError``: mode ``"timediff"`` (the reference's broadcast of a ``(B,)``
mean against ``(B, T−1, C, H, W)`` only works for B ∈ {1, W} and nothing consumes its result on this path); any other unknown mode
string (the reference falls through to un-normalised weights of shape ``(T,)``); ``from_params`` with ``params.lat`` / ``params.lon``
(the ``GridConverter`` branch).  Noise in ``"perturb"`` mode is the noise stage's out-of-place add on the window in front of the
kernels (torch glue, not fused).  Noise without cached unpredicted features goes behind ``x`` (``InputNoise``'s rule).
"""
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, dtype_code, lib, ptr, stream

_FILE_KEYS = ("add_orography", "add_landmask", "add_soiltype", "add_copernicus_emb")          # planes the reference reads from files


# ---- launches -------------------------------------------------------------------------------------------------------------
def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("makani_amd Preprocessor2D runs on the GPU (HIP) path only")


def _prep(t):
    if t is None:
        return None
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    return t.contiguous()


class _Src:
    """the three source tensors of the kernels and their sizes; ``win`` (B, T·C, H, W), ``unp`` (B, T, U, H, W), ``noi`` (B, T, N, H, W).
    In backward the unpredicted features (and a noise that gets no gradient) are absent and ``U`` / ``N`` name their channels."""

    def __init__(self, win, unp, noi, T, U=None, N=None):
        _need_gpu(win)
        self.win, self.unp, self.noi = _prep(win), _prep(unp), _prep(noi)
        self.T = int(T)
        self.B, self.WC = self.win.shape[0], self.win.shape[1]
        self.hw_shape = tuple(self.win.shape[-2:])
        self.hw = self.hw_shape[0] * self.hw_shape[1]
        if self.win.dim() != 4 or self.WC % self.T:
            raise RuntimeError(f"an input of shape {tuple(self.win.shape)}: expected (B, T·C, H, W) with the channel dim divisible by "
                               f"n_history + 1 = {self.T}")
        self.C = self.WC // self.T
        for name, t in (("unpredicted features", self.unp), ("noise", self.noi)):
            if t is not None and (t.dim() != 5 or t.shape[0] != self.B or t.shape[1] != self.T or tuple(t.shape[-2:]) != self.hw_shape):
                raise RuntimeError(f"the {name} have shape {tuple(t.shape)}, expected ({self.B}, {self.T}, *, {self.hw_shape[0]}, "
                                   f"{self.hw_shape[1]}) next to an input of shape {tuple(self.win.shape)}")
        self.U = (0 if self.unp is None else self.unp.shape[2]) if U is None else U
        self.N = (0 if self.noi is None else self.noi.shape[2]) if N is None else N
        self.J = self.C + self.U + self.N

    def args(self):
        f32 = _lib.MK_F32
        return (ptr(self.win), dtype_code(self.win), ptr(self.unp), f32 if self.unp is None else dtype_code(self.unp),
                ptr(self.noi), f32 if self.noi is None else dtype_code(self.noi))

    def dims(self):
        return self.B, self.T, self.WC, self.U, self.N


def _chunks(hw):
    return lib().mk_prep_chunks(hw)


def _stats(src, q, wt, tri=False):
    """(mu, sigma) (B, J) fp32, or the fp64 triple (B, J, 3) = (Σω, mean, M2) of this rank's shard"""
    dev = src.win.device
    ws = torch.empty(src.B * src.J * _chunks(src.hw) * 4, dtype=torch.float32, device=dev)
    if tri:
        out = torch.empty((src.B, src.J, 3), dtype=torch.float64, device=dev)
        mu = sigma = None
    else:
        out = None
        mu = torch.empty((src.B, src.J), dtype=torch.float32, device=dev)
        sigma = torch.empty_like(mu)
    check(lib().mk_prep_stats(*src.args(), ptr(q), ptr(wt), ptr(mu), ptr(sigma), ptr(out), ptr(ws), *src.dims(), src.hw, stream()),
          "mk_prep_stats")
    return out if tri else (mu, sigma)


def _merge_ranks(tri):
    """Chan's merge of the ranks' (Σω, mean, M2) (R, B, J, 3) fp64 in rank order -> (mu, sigma) fp32"""
    W, mean, M2 = tri[0, ..., 0], tri[0, ..., 1], tri[0, ..., 2]
    for r in range(1, tri.shape[0]):
        w, m, m2 = tri[r, ..., 0], tri[r, ..., 1], tri[r, ..., 2]
        Wn = W + w
        delta = m - mean
        mean = mean + delta * (w / Wn)
        M2 = M2 + m2 + delta * delta * (W * w / Wn)
        W = Wn
    return (W * mean).float().contiguous(), torch.sqrt(M2).float().contiguous()


def _stats_any(src, q, wt, dist):
    if not dist:
        return _stats(src, q, wt)
    from . import distributed as thd
    from .ops import _all_gather_stack
    return _merge_ranks(_all_gather_stack(_stats(src, q, wt, tri=True), thd.spatial_group()))


def _reduce_G(G, dist):
    if dist:
        from . import distributed as thd
        from .ops import _all_reduce_sum
        _all_reduce_sum(G, thd.spatial_group())
    return G


def _assemble(src, stat, mu, sigma):
    S = 0 if stat is None else stat.shape[-3]
    out = torch.empty((src.B, src.T * src.J + S, *src.hw_shape), dtype=src.win.dtype, device=src.win.device)
    check(lib().mk_prep_assemble(*src.args(), ptr(stat), _lib.MK_F32 if stat is None else dtype_code(stat), ptr(mu), ptr(sigma), ptr(out),
                                 dtype_code(out), *src.dims(), S, src.hw, stream()), "mk_prep_assemble")
    return out


def _bwd_sums(g, src, S, mu, sigma, gmu, gsig, need_win, need_noi):
    """G (2, B, J) = (gmu - Σg/σ, gsig - Σ g xn/σ); the sums only for the channels that get a gradient"""
    G = torch.empty((2, src.B, src.J), dtype=torch.float32, device=g.device)
    ws = torch.empty(src.B * src.J * _chunks(src.hw) * 2, dtype=torch.float32, device=g.device)
    check(lib().mk_prep_bwd_sums(ptr(g), dtype_code(g), *src.args(), ptr(mu), ptr(sigma), ptr(gmu), ptr(gsig), ptr(G), ptr(ws),
                                 *src.dims(), S, int(need_win) | 2 * int(need_noi), src.hw, stream()), "mk_prep_bwd_sums")
    return G


def _bwd_apply(g, src, S, q, wt, mu, sigma, G, need_win, need_noi):
    dwin = torch.empty_like(src.win) if need_win else None
    dnoi = torch.empty_like(src.noi) if need_noi else None
    if need_win or need_noi:
        check(lib().mk_prep_bwd_apply(ptr(g), _lib.MK_F32 if g is None else dtype_code(g), *src.args(), ptr(q), ptr(wt), ptr(mu),
                                      ptr(sigma), ptr(G), ptr(dwin), ptr(dnoi), *src.dims(), S, src.hw, stream()), "mk_prep_bwd_apply")
    return dwin, dnoi


def _flat_stat(g):
    return None if g is None else g.reshape(g.shape[0], g.shape[1]).float().contiguous()


def _as_grad(g):
    return g if g.dtype in (torch.float32, torch.bfloat16) and g.is_contiguous() else _prep(g)


def _save(ctx, src, *extra):
    """what backward reads: the window, and the noise only when it gets a gradient.  The unpredicted features (updated in place by
    ``append_history``) and a noise buffer without gradient (updated in place by its process) are not kept."""
    need_noi = src.noi is not None and ctx.needs_input_grad[2]
    ctx.save_for_backward(src.win, src.noi if need_noi else None, *extra)
    ctx.meta = (src.T, src.U, src.N)


def _load(ctx):
    win, noi, *extra = ctx.saved_tensors
    T, U, N = ctx.meta
    return _Src(win, None, noi, T, U=U, N=N), ctx.needs_input_grad[0], noi is not None, extra


class _GatherFn(torch.autograd.Function):
    """out (B, T·J + S, H, W) = the channels of the sources per time level, then the static planes; no normalisation"""

    @staticmethod
    def forward(ctx, win, unp, noi, stat, T):
        src = _Src(win, unp, noi, T)
        _save(ctx, src)
        ctx.S = 0 if stat is None else stat.shape[-3]
        return _assemble(src, stat, None, None)

    @staticmethod
    def backward(ctx, g):
        src, need_win, need_noi, _ = _load(ctx)
        dwin, dnoi = _bwd_apply(_as_grad(g), src, ctx.S, None, None, None, None, None, need_win, need_noi)
        return dwin, None, dnoi, None, None


class _StatsFn(torch.autograd.Function):
    """(mu, sigma) (B, J, 1, 1) of the sources"""

    @staticmethod
    def forward(ctx, win, unp, noi, q, wt, T, dist):
        src = _Src(win, unp, noi, T)
        mu, sigma = _stats_any(src, q, wt, dist)
        _save(ctx, src, q, wt, mu, sigma)
        ctx.dist = dist
        return mu.view(src.B, src.J, 1, 1), sigma.view(src.B, src.J, 1, 1)

    @staticmethod
    def backward(ctx, gmu, gsig):
        src, need_win, need_noi, (q, wt, mu, sigma) = _load(ctx)
        zero = torch.zeros((src.B, src.J), dtype=torch.float32, device=mu.device)
        G = torch.stack([zero if gmu is None else _flat_stat(gmu), zero if gsig is None else _flat_stat(gsig)])
        G = _reduce_G(G.contiguous(), ctx.dist)          # copy_to_parallel_region's backward
        dwin, dnoi = _bwd_apply(None, src, 0, q, wt, mu, sigma, G, need_win, need_noi)
        return dwin, None, dnoi, None, None, None, None


class _NormFn(torch.autograd.Function):
    """xn = (x - mu) / sigma on x (B, T·J, H, W) with mu, sigma (B, J, 1, 1): ``history_normalize``"""

    @staticmethod
    def forward(ctx, x, mu, sigma, T):
        src = _Src(x, None, None, T)
        mu, sigma = _flat_stat(mu), _flat_stat(sigma)
        if tuple(mu.shape) != (src.B, src.J):
            raise RuntimeError(f"history statistics of shape {tuple(mu.shape)} next to {src.J} channels per time level")
        ctx.T = src.T
        ctx.save_for_backward(src.win, mu, sigma)
        return _assemble(src, None, mu, sigma)

    @staticmethod
    def backward(ctx, g):
        x, mu, sigma = ctx.saved_tensors
        src = _Src(x, None, None, ctx.T)
        g = _as_grad(g)
        dmu = dsig = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            G = _bwd_sums(g, src, 0, mu, sigma, None, None, True, False)
            dmu, dsig = G[0].view(src.B, src.J, 1, 1), G[1].view(src.B, src.J, 1, 1)
        dx, _ = _bwd_apply(g, src, 0, None, None, mu, sigma, None, ctx.needs_input_grad[0], False)
        return dx, dmu, dsig, None


class _NormAssembleFn(torch.autograd.Function):
    """(out, mu, sigma): statistics of the sources, then the whole network input in one launch"""

    @staticmethod
    def forward(ctx, win, unp, noi, stat, q, wt, T, dist):
        src = _Src(win, unp, noi, T)
        mu, sigma = _stats_any(src, q, wt, dist)
        _save(ctx, src, q, wt, mu, sigma)
        ctx.dist, ctx.S = dist, 0 if stat is None else stat.shape[-3]
        return _assemble(src, stat, mu, sigma), mu.view(src.B, src.J, 1, 1), sigma.view(src.B, src.J, 1, 1)

    @staticmethod
    def backward(ctx, g, gmu, gsig):
        src, need_win, need_noi, (q, wt, mu, sigma) = _load(ctx)
        if not (need_win or need_noi):
            return (None,) * 8
        if g is None:
            g = torch.zeros((src.B, src.T * src.J + ctx.S, *src.hw_shape), dtype=src.win.dtype, device=mu.device)
        g = _as_grad(g)
        G = _reduce_G(_bwd_sums(g, src, ctx.S, mu, sigma, _flat_stat(gmu), _flat_stat(gsig), need_win, need_noi), ctx.dist)
        dwin, dnoi = _bwd_apply(g, src, ctx.S, q, wt, mu, sigma, G, need_win, need_noi)
        return dwin, None, dnoi, None, None, None, None, None


def _finish(yn, bias, mu, sigma, J):
    B, Cout = yn.shape[0], yn.shape[1]
    y = torch.empty_like(yn)
    check(lib().mk_prep_finish(ptr(yn), dtype_code(yn), ptr(bias), ptr(mu), ptr(sigma), ptr(y), B, Cout, J, yn.shape[-2] * yn.shape[-1],
                               stream()), "mk_prep_finish")
    return y


class _FinishFn(torch.autograd.Function):
    """y = (yn - bias) sigma[:, :Cout] + mu[:, :Cout]; ``bias`` (Cout, H, W) or None, ``mu`` / ``sigma`` (B, J, 1, 1) or None"""

    @staticmethod
    def forward(ctx, yn, bias, mu, sigma):
        _need_gpu(yn)
        yn = _prep(yn)
        norm = mu is not None
        J = mu.shape[1] if norm else yn.shape[1]
        if norm:
            mu, sigma = _flat_stat(mu), _flat_stat(sigma)
            if mu.shape[1] < yn.shape[1]:
                raise RuntimeError(f"history statistics of {mu.shape[1]} channels next to a prediction of {yn.shape[1]}")
        ctx.J, ctx.norm = J, norm
        ctx.save_for_backward(yn, bias, sigma)
        return _finish(yn, bias, mu, sigma, J)

    @staticmethod
    def backward(ctx, g):
        yn, bias, sigma = ctx.saved_tensors
        g = _as_grad(g)
        if g.dtype != yn.dtype:
            g = g.to(yn.dtype)
        B, Cout, J = yn.shape[0], yn.shape[1], ctx.J
        dyn = dmu = dsig = None
        if ctx.needs_input_grad[0]:
            dyn = _finish(g, None, None, sigma, J) if ctx.norm else g
        if ctx.norm and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]):
            hw = yn.shape[-2] * yn.shape[-1]
            out = torch.zeros((2, B, J), dtype=torch.float32, device=g.device)
            ws = torch.empty(B * Cout * _chunks(hw) * 2, dtype=torch.float32, device=g.device)
            check(lib().mk_prep_finish_bwd(ptr(g), dtype_code(g), ptr(yn), dtype_code(yn), ptr(bias), ptr(out[0]), ptr(out[1]), ptr(ws),
                                           B, Cout, J, hw, stream()), "mk_prep_finish_bwd")
            dmu, dsig = out[0].view(B, J, 1, 1), out[1].view(B, J, 1, 1)
        return dyn, None, dmu, dsig


# ---- the module -----------------------------------------------------------------------------------------------------------
def grid_static_features(params):
    """the ``add_grid`` planes of ``preprocessor_helpers.get_static_features`` (:128-187): the linspace grid, ``gridtype``
    "sinusoidal" with ``grid_num_frequencies`` / ``add_cos_to_grid``, ``normalize_static_features`` and the ``img_local_*`` slice"""
    get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
    if hasattr(params, "lat") and hasattr(params, "lon"):
        raise NotImplementedError("add_grid with params.lat / params.lon (the GridConverter branch) is not ported: drop lat / lon "
                                  "for the linspace grid, or pass the planes through static_features=")
    H, W = params.img_shape_x, params.img_shape_y
    with torch.no_grad():
        tx = torch.linspace(0, 1, H + 1, dtype=torch.float32)[0:-1]
        ty = torch.linspace(0, 1, W + 1, dtype=torch.float32)[0:-1]
        xg, yg = torch.meshgrid(tx, ty, indexing="ij")
        grid = torch.cat([xg.unsqueeze(0).unsqueeze(0), yg.unsqueeze(0).unsqueeze(0)], dim=1)
        if get("gridtype", "sinusoidal") == "sinusoidal":
            planes = []
            for freq in range(1, get("grid_num_frequencies", 1) + 1):
                arg = grid if freq == 1 else freq * grid
                planes += [torch.sin(arg), torch.cos(arg)] if get("add_cos_to_grid", True) else [torch.sin(arg)]
            static = torch.cat(planes, dim=-3)
        else:
            static = grid
        if get("normalize_static_features", False):
            from .losses import _rule_weights, grid_to_quadrature_rule
            q = _rule_weights(grid_to_quadrature_rule(get("data_grid_type", "equiangular")), params.img_shape) / (4.0 * math.pi)
            ch, cw = get("img_crop_shape_x", H), get("img_crop_shape_y", W)
            oh, ow = get("img_crop_offset_x", 0), get("img_crop_offset_y", 0)
            q = q[oh:oh + ch, ow:ow + cw].float().reshape(1, 1, ch, cw)
            mean = torch.sum(static * q, dim=(-2, -1)).reshape(1, -1, 1, 1)
            std = torch.sqrt(torch.sum(torch.square(static - mean) * q, dim=(-2, -1)).reshape(1, -1, 1, 1))
            static = (static - mean) / std
        x0, y0 = get("img_local_offset_x", 0), get("img_local_offset_y", 0)
        x1, y1 = min(x0 + get("img_local_shape_x", H), H), min(y0 + get("img_local_shape_y", W), W)
        sub = get("subsampling_factor", 1)
        return static[:, :, x0:x1:sub, y0:y1:sub].contiguous()


class Preprocessor2D(nn.Module):
    """See the module docstring.  ``Preprocessor2D(img_shape=, n_history=0, history_normalization_mode="none",
    history_normalization_decay=None, grid_type="equiangular", static_features=None, bias_correction=None, input_noise=None,
    spatial_distributed=False)`` or ``Preprocessor2D.from_params(params, static_features=None, bias_correction=None)``.
    ``static_features`` (1, S, H, W), ``bias_correction`` (1, C_out, H, W), ``input_noise`` a ``makani_amd.noise.InputNoise``."""

    def __init__(self, *, img_shape, n_history=0, history_normalization_mode="none", history_normalization_decay=None,
                 grid_type="equiangular", static_features=None, bias_correction=None, input_noise=None, spatial_distributed=False):
        super().__init__()
        self.img_shape = [int(img_shape[0]), int(img_shape[1])]
        self.n_history = int(n_history)
        T = self.n_history + 1
        mode = history_normalization_mode
        self.history_normalization_mode = mode
        if mode == "exponential":
            if history_normalization_decay is None:
                raise ValueError("history_normalization_mode 'exponential' needs history_normalization_decay")
            self.history_normalization_decay = history_normalization_decay
            w = torch.exp((-history_normalization_decay) * torch.arange(start=self.n_history, end=-1, step=-1, dtype=torch.float32))
            w = w / torch.sum(w)
            weights, wt = torch.reshape(w, (1, -1, 1, 1, 1)), w.clone()
        elif mode == "mean":
            w = torch.as_tensor(1.0 / float(T), dtype=torch.float32)
            weights, wt = torch.reshape(w, (1, -1, 1, 1, 1)), w.repeat(T)
        elif mode == "none":
            weights, wt = torch.ones(T, dtype=torch.float32), None
        elif mode == "timediff":
            raise NotImplementedError("history_normalization_mode 'timediff': the reference's broadcast of a (B,) mean against "
                                      "(B, T-1, C, H, W) only works for B in {1, W}, and nothing consumes its result on this path")
        else:
            raise NotImplementedError(f"history_normalization_mode {mode!r}: the reference falls through to un-normalised weights of "
                                      f"shape (T,) for it; supported: 'none', 'mean', 'exponential'")
        self.register_buffer("history_normalization_weights", weights, persistent=False)
        self.spatial_distributed = False
        if mode != "none":
            from .losses import GridQuadrature, grid_to_quadrature_rule
            self.register_buffer("history_time_weights", wt, persistent=False)
            self.quadrature = GridQuadrature(grid_to_quadrature_rule(grid_type), img_shape=self.img_shape, crop_shape=None,
                                             crop_offset=(0, 0), normalize=True, distributed=bool(spatial_distributed))
            self.spatial_distributed = self.quadrature.distributed
        self.history_mean = None
        self.history_std = None
        self.history_eps = 1e-6
        self.unpredicted_inp_train = None
        self.unpredicted_tar_train = None
        self.unpredicted_inp_eval = None
        self.unpredicted_tar_eval = None
        if bias_correction is not None:
            if bias_correction.dim() != 4 or bias_correction.shape[0] != 1:
                raise ValueError(f"bias_correction has shape {tuple(bias_correction.shape)}, expected (1, C_out, H, W)")
            self.register_buffer("bias_correction", bias_correction.detach().to(torch.float32).contiguous(), persistent=False)
        self.do_add_static_features = False
        if static_features is not None:
            if static_features.dim() != 4 or static_features.shape[0] != 1:
                raise ValueError(f"static_features has shape {tuple(static_features.shape)}, expected (1, S, H, W)")
            self.do_add_static_features = True
            self.register_buffer("static_features", static_features.detach().to(torch.float32).contiguous(), persistent=False)
        if input_noise is not None and input_noise.n_history != self.n_history:
            raise ValueError(f"input_noise carries n_history = {input_noise.n_history}, the preprocessor {self.n_history}")
        self.noise_stage = input_noise

    @classmethod
    def from_params(cls, params, static_features=None, bias_correction=None):
        """The preprocessor ``Preprocessor2D(params)`` of the reference builds (``preprocessor.py:84-232``): ``n_history``,
        ``history_normalization_mode`` / ``_decay``, ``model_grid_type``, ``img_shape_x/y_resampled``, ``input_noise`` (through
        ``InputNoise.from_params``) and the ``add_grid`` planes (``grid_static_features``).  The file-backed fields come in as
        tensors: ``static_features`` holds the planes of ``add_orography`` / ``add_landmask`` / ``add_soiltype`` /
        ``add_copernicus_emb`` in the reference's order (they go behind the grid planes), ``bias_correction`` the field of
        ``params.bias_correction``; file I/O stays with the caller."""
        get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
        wanted = [key for key in _FILE_KEYS if get(key, False)]
        if wanted and static_features is None:
            raise ValueError(f"params.{wanted[0]} is set: this package reads no files — load the field and pass the planes through "
                             f"the static_features= keyword")
        if get("bias_correction", None) is not None and bias_correction is None:
            raise ValueError("params.bias_correction is set: this package reads no files — load the field and pass it through the "
                             "bias_correction= keyword")
        static = grid_static_features(params) if get("add_grid", False) else None
        if static_features is not None:
            static = static_features if static is None else torch.cat([static, static_features.to(static.dtype)], dim=1)
        noise = None
        if get("input_noise", None) is not None:
            from .noise import InputNoise
            noise = InputNoise.from_params(params)
        from . import comm
        return cls(img_shape=(params.img_shape_x_resampled, params.img_shape_y_resampled), n_history=params.n_history,
                   history_normalization_mode=get("history_normalization_mode", "none"),
                   history_normalization_decay=get("history_normalization_decay", None),
                   grid_type=get("model_grid_type", "equiangular"), static_features=static, bias_correction=bias_correction,
                   input_noise=noise, spatial_distributed=comm.get_size("spatial") > 1)

    # ---- history layout (preprocessor.py:234-295) ----
    def flatten_history(self, x):
        if x.dim() == 5:
            b_, t_, c_, h_, w_ = x.shape
            x = torch.reshape(x, (b_, t_ * c_, h_, w_))
        return x

    def expand_history(self, x, nhist):
        if x.dim() == 4:
            b_, ct_, h_, w_ = x.shape
            if ct_ % nhist:
                raise RuntimeError(f"expand_history: channel dim {ct_} is not divisible by nhist={nhist}. The flattened-history input "
                                   f"may not match the preprocessor's expected n_history={self.n_history} (so ct_ should be a "
                                   f"multiple of n_history+1={nhist}).")
            x = torch.reshape(x, (b_, nhist, ct_ // nhist, h_, w_))
        return x

    # ---- static features (preprocessor.py:297-339, 969-982) ----
    def _static(self):
        if not self.do_add_static_features:
            return None
        if self.static_features.requires_grad:
            raise RuntimeError("static_features requires grad: the preprocessor gives gradients to the window and the noise only")
        return self.static_features[0]

    def add_static_features(self, x):
        if self.do_add_static_features:
            x = _GatherFn.apply(x, None, None, self._static(), 1)
        return x

    def remove_static_features(self, x):
        if self.do_add_static_features:
            nfeat = self.static_features.shape[1]
            x = x[:, : x.shape[1] - nfeat, :, :]
        return x

    def get_static_features(self):
        return self.static_features.clone() if self.do_add_static_features else None

    # ---- unpredicted features (preprocessor.py:341-464, 689-746, 930-1016) ----
    def _unpredicted(self, target=False):
        if self.training:
            return self.unpredicted_tar_train if target else self.unpredicted_inp_train
        return self.unpredicted_tar_eval if target else self.unpredicted_inp_eval

    def append_history(self, x1, x2, step, update_state=True):
        if update_state:
            inp, tar = ("unpredicted_inp_train", "unpredicted_tar_train") if self.training else ("unpredicted_inp_eval", "unpredicted_tar_eval")
            utar_all, uinp = getattr(self, tar), getattr(self, inp)
            if (utar_all is not None) and (step < utar_all.shape[1]):
                utar = utar_all[:, step:(step + 1), :, :, :]
                if self.n_history == 0:
                    uinp.copy_(utar)
                else:
                    uinp.copy_(torch.cat([uinp[:, 1:, :, :, :], utar], dim=1))
        if self.n_history > 0:
            x1 = self.expand_history(x1, nhist=self.n_history + 1)
            x2 = self.expand_history(x2, nhist=1)
            res = self.flatten_history(torch.cat([x1[:, 1:, :, :, :], x2], dim=1))
        else:
            res = x2
        return res

    def _ensure_cached(self, name, tensor):
        current = getattr(self, name)
        if tensor is None:
            setattr(self, name, None)
            return
        if (current is not None) and (current.shape == tensor.shape):
            current.copy_(tensor)
        else:
            setattr(self, name, tensor.clone())

    def cache_unpredicted_features(self, x, y, xz=None, yz=None):
        if self.training:
            self._ensure_cached("unpredicted_inp_train", xz)
            self._ensure_cached("unpredicted_tar_train", yz)
        else:
            self._ensure_cached("unpredicted_inp_eval", xz)
            self._ensure_cached("unpredicted_tar_eval", yz)
        return x, y

    def get_unpredicted_features(self):
        inpu, taru = self._unpredicted(False), self._unpredicted(True)
        return (None if inpu is None else inpu.clone()), (None if taru is None else taru.clone())

    def _sources(self, x, xc, with_noise=True):
        """the window (flattened, perturbed when the noise says so), the unpredicted features and the noise channels of ``x``"""
        T = self.n_history + 1
        if xc is not None:
            if xc.requires_grad:
                raise RuntimeError("the cached unpredicted features require grad: the preprocessor gives gradients to the window and "
                                   "the noise only")
            if x.shape[0] != xc.shape[0]:
                raise RuntimeError(f"_append_channels: batch mismatch between input ({x.shape[0]}) and cached unpredicted features "
                                   f"({xc.shape[0]}). Did you cache xz/yz at a different batch size than the current forward?")
            xc = self.expand_history(xc, T)
        win, noi = self.flatten_history(x), None
        stage = self.noise_stage if with_noise else None
        if stage is not None:
            if stage.input_noise_mode == "concatenate":
                noi = stage.input_noise()
                if noi.shape[0] != x.shape[0]:
                    raise RuntimeError(f"batch mismatch between input_noise state ({noi.shape[0]}) and input ({x.shape[0]}). Did you "
                                       f"call update_internal_state(batch_size=...) at a different batch than the current forward pass?")
            else:
                win = stage(win)          # "perturb": the stage's out-of-place add on the window
        return win, xc, noi

    def _append_channels(self, x, xc):
        xdim = x.dim()
        T = self.n_history + 1
        win, xc, noi = self._sources(x, xc)
        if xc is None and noi is None:
            xo = win
        else:
            xo = _GatherFn.apply(win, xc, noi, None, T)
        return xo if xdim == 4 else self.expand_history(xo, T)

    def append_unpredicted_features(self, inp, target=False):
        xc = self._unpredicted(target)
        if xc is not None or self.noise_stage is not None:          # (noise without cached features goes behind x)
            inp = self._append_channels(inp, xc)
        return inp

    # ---- history normalisation (preprocessor.py:466-687) ----
    def history_compute_stats(self, x):
        if self.history_normalization_mode == "none":
            self.history_mean = torch.zeros((1, 1, 1, 1), dtype=torch.float32, device=x.device)
            self.history_std = torch.ones((1, 1, 1, 1), dtype=torch.float32, device=x.device)
            return
        _need_gpu(x)
        self.history_mean, self.history_std = _StatsFn.apply(self.flatten_history(x), None, None, self.quadrature.quad_weight,
                                                             self.history_time_weights, self.n_history + 1, self.spatial_distributed)

    def _check_history_stats(self, x, caller):
        if self.history_mean is None or self.history_std is None:
            raise RuntimeError(f"{caller}: history_mean / history_std are None. Call history_compute_stats(x) before {caller} "
                               f"(mode='{self.history_normalization_mode}').")
        stats_batch = self.history_mean.shape[0]
        if stats_batch != x.shape[0]:
            raise RuntimeError(f"{caller}: batch mismatch between input ({x.shape[0]}) and cached history stats ({stats_batch}). "
                               f"Did you forget to call history_compute_stats on the current input before {caller}?")

    def _target_stats(self, x):
        c = x.shape[1]
        return self.history_mean[:, :c, :, :], self.history_std[:, :c, :, :]

    def history_normalize(self, x, target=False):
        if self.history_normalization_mode in ["none", "timediff"]:
            return x
        self._check_history_stats(x, caller="history_normalize")
        xshape = x.shape
        x = self.flatten_history(x)
        if target:
            xn = _NormFn.apply(x, *self._target_stats(x), 1)
        else:
            xn = _NormFn.apply(x, self.history_mean, self.history_std, self.n_history + 1)
        return torch.reshape(xn, xshape) if len(xshape) == 5 else xn

    def history_denormalize(self, xn, target=False):
        if self.history_normalization_mode in ["none", "timediff"]:
            return xn
        self._check_history_stats(xn, caller="history_denormalize")
        xnshape = xn.shape
        xn = self.flatten_history(xn)
        if target:
            x = _FinishFn.apply(xn, None, self.history_mean, self.history_std)
        else:
            T = self.n_history + 1
            x = _FinishFn.apply(xn, None, torch.tile(self.history_mean, (1, T, 1, 1)), torch.tile(self.history_std, (1, T, 1, 1)))
        return torch.reshape(x, xnshape) if len(xnshape) == 5 else x

    # ---- bias correction (preprocessor.py:1018-1036) ----
    def _bias(self):
        bias = getattr(self, "bias_correction", None)
        if bias is not None and bias.requires_grad:
            raise RuntimeError("bias_correction requires grad: the preprocessor gives gradients to the window and the noise only")
        return None if bias is None else bias[0]

    def correct_bias(self, inp):
        bias = self._bias()
        if bias is not None:
            if tuple(inp.shape[1:]) != tuple(bias.shape):
                raise RuntimeError(f"correct_bias: the input has shape {tuple(inp.shape)}, the bias correction {tuple(bias.shape)}")
            inp = _FinishFn.apply(inp, bias, None, None)
        return inp

    # ---- noise state (preprocessor.py:872-928) ----
    def update_internal_state(self, replace_state=False, batch_size=None):
        if self.noise_stage is not None:
            self.noise_stage.update_internal_state(replace_state=replace_state, batch_size=batch_size)

    # ---- the fused entry points ----
    @_lib.device_guard
    def assemble(self, inp):
        """``inp`` (B, T·C, H, W) -> the network input (B, T·J + S, H, W); sets ``history_mean`` / ``history_std``"""
        win, xc, noi = self._sources(inp, self._unpredicted(False))
        T = self.n_history + 1
        stat = self._static()
        if self.history_normalization_mode == "none":
            self.history_compute_stats(win)
            if xc is None and noi is None and stat is None:
                return win
            return _GatherFn.apply(win, xc, noi, stat, T)
        out, self.history_mean, self.history_std = _NormAssembleFn.apply(win, xc, noi, stat, self.quadrature.quad_weight,
                                                                         self.history_time_weights, T, self.spatial_distributed)
        return out

    @_lib.device_guard
    def finish(self, yn):
        """``yn`` (B, C_out, H, W) -> ``history_denormalize(correct_bias(yn), target=True)`` in one launch"""
        bias = self._bias()
        if self.history_normalization_mode == "none":
            return yn if bias is None else self.correct_bias(yn)
        self._check_history_stats(yn, caller="history_denormalize")
        if bias is not None and tuple(yn.shape[1:]) != tuple(bias.shape):
            raise RuntimeError(f"correct_bias: the input has shape {tuple(yn.shape)}, the bias correction {tuple(bias.shape)}")
        return _FinishFn.apply(yn, bias, self.history_mean, self.history_std)
