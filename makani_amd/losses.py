"""Drop-in geometric losses on the HIP path.

``GridQuadrature`` mirrors ``makani/utils/grids.py:102-191`` (same constructor, same non-persistent
``quad_weight`` buffer, ``forward(x)`` = quadrature over the last two axes) and ``GeometricLpLoss`` mirrors
``makani/utils/losses/lp_loss.py:28-107`` (``abs`` / ``rel`` / ``forward(prd, tar, wgt)`` -> (B, C) norms).
The elementwise chain ``|prd - tar|^p * wgt * q`` and the plane reduction are ONE HIP kernel
(``mk_quad_lp_fwd``), its autograd one more (``mk_quad_lp_bwd``); prediction and target may have different
dtypes (bf16 prediction, fp32 target) without a cast pass.  Spatially distributed quadrature sums over the
"spatial" group of ``makani_amd.distributed``.
"""
import contextlib
import math
from functools import partial
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, legendre
from ._lib import device_guard, check, dtype_code, lib, need_gpu, prep, ptr, stream
from .constraints import MAX_LEVELS as MAX_HYDRO_LEVELS, Q_CORRECTION_MOIST_AIR, R_DRY_AIR, _Tabled, get_matching_channels_pl
from .ensemble import MAX_ENSEMBLE          # noqa: F401  (importable from here as before)
from .ensemble import (ReduceFromGroupFn, check_forecast_dims, check_weight_dims, ensemble_active, ensemble_size_check,
                       ensemble_split, flatten_and_split)

GRID_TO_QUADRATURE_RULE = {
    "euclidean": "uniform",
    "equiangular": "naive",
    "legendre-gauss": "legendre-gauss",
    "clenshaw-curtiss": "clenshaw-curtiss",
    "weatherbench2": "weatherbench2",
}


def grid_to_quadrature_rule(grid_type: str) -> str:
    """``makani/utils/grids.py:27-40``."""
    if grid_type not in GRID_TO_QUADRATURE_RULE:
        raise NotImplementedError(f"Grid type {grid_type} does not have a quadrature rule")
    return GRID_TO_QUADRATURE_RULE[grid_type]


def _quad_launch(a, b, wgt, q, mode, p):
    """sums (planes,) f32 of q * (mode ? |a-b|^p : a) * wgt over the trailing (H, W) plane."""
    planes = a.numel() // q.numel()
    hw = q.numel()
    ch = lib().mk_quad_lp_chunks(hw)
    sums = torch.empty((2, planes), dtype=torch.float32, device=a.device)
    ws = torch.empty((planes * ch * 2,), dtype=torch.float32, device=a.device)
    check(lib().mk_quad_lp_fwd(ptr(a), dtype_code(a), ptr(b) if b is not None else None,
                               dtype_code(b) if b is not None else _lib.MK_F32, ptr(wgt) if wgt is not None else None,
                               ptr(q), ptr(sums), ptr(ws), planes, hw, mode, float(p), stream()), "mk_quad_lp_fwd")
    return sums[0]


class QuadLpFn(torch.autograd.Function):
    """out[...] = sum_{h,w} q[h,w] * (mode ? |a - b|^p : a) * wgt;  a, b: (..., H, W)."""

    @staticmethod
    def forward(ctx, a, b, wgt, q, mode, p):
        need_gpu(a)
        a = prep(a)
        b = prep(b, a.shape) if b is not None else None
        w = prep(wgt, a.shape).float() if wgt is not None else None
        ctx.save_for_backward(a, b, w, q)
        ctx.meta = (mode, float(p))
        return _quad_launch(a, b, w, q, mode, p).view(a.shape[:-2])

    @staticmethod
    def backward(ctx, g):
        a, b, w, q = ctx.saved_tensors
        mode, p = ctx.meta
        g = g.contiguous().float().view(-1)
        need_a, need_b = ctx.needs_input_grad[0], (b is not None and ctx.needs_input_grad[1])
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        if need_a or need_b:
            check(lib().mk_quad_lp_bwd(ptr(a), dtype_code(a), ptr(b) if b is not None else None,
                                       dtype_code(b) if b is not None else _lib.MK_F32,
                                       ptr(w) if w is not None else None, ptr(q), ptr(g),
                                       ptr(da) if need_a else None, ptr(db) if need_b else None,
                                       g.numel(), q.numel(), mode, p, stream()), "mk_quad_lp_bwd")
        return da, db, None, None, None, None


def _rule_weights(rule: str, img_shape) -> torch.Tensor:
    """(H, W) weights summing to 4 pi (before normalisation), ``grids.py:111-144``; same torch-fp32 arithmetic
    for the closed-form rules so the buffer is bit-identical to the reference's."""
    H, W = img_shape
    dlambda = 2 * math.pi / W
    if rule == "naive":
        jac = torch.clamp(torch.sin(torch.linspace(0, math.pi, H)), min=0.0)
        q = ((dlambda * (math.pi / H)) * jac.unsqueeze(1)).tile(1, W)
        return q * (4.0 * math.pi) / torch.sum(q)
    if rule in ("clenshaw-curtiss", "legendre-gauss"):
        _, w = legendre.clenshaw_curtis(H) if rule == "clenshaw-curtiss" else legendre.gauss_legendre(H)
        return (dlambda * torch.from_numpy(w.copy()).unsqueeze(1)).tile(1, W)
    if rule == "weatherbench2":
        lats = torch.linspace(0, math.pi, H)
        bounds = torch.cat([torch.zeros(1), (lats[:-1] + lats[1:]) / 2, torch.full((1,), math.pi)])
        jac = torch.cos(bounds[:-1]) - torch.cos(bounds[1:])
        return (dlambda * jac.unsqueeze(1)).tile(1, W)
    if rule == "uniform":
        q = torch.ones((H, W))
        return 4.0 * math.pi * q / torch.sum(q)
    raise ValueError(f"Unknown quadrature rule {rule}")


class GridQuadrature(nn.Module):
    def __init__(self, quadrature_rule, img_shape, crop_shape=None, crop_offset=(0, 0), normalize=False, distributed=False):
        super().__init__()
        from . import distributed as thd
        self.distributed = bool(distributed) and thd.ensure_initialized()
        crop_shape = img_shape if crop_shape is None else crop_shape
        q = _rule_weights(quadrature_rule, img_shape)
        if normalize:
            q = q / (4.0 * math.pi)
        h0, hl = crop_offset[0], crop_shape[0]
        w0, wl = crop_offset[1], crop_shape[1]
        if self.distributed:        # this rank's lat/lon shard of the crop (grids.py:150-168)
            if thd.polar_group_size() > 1:
                sh = thd.compute_split_shapes(crop_shape[0], thd.polar_group_size())
                h0, hl = h0 + sum(sh[: thd.polar_group_rank()]), sh[thd.polar_group_rank()]
            if thd.azimuth_group_size() > 1:
                sw = thd.compute_split_shapes(crop_shape[1], thd.azimuth_group_size())
                w0, wl = w0 + sum(sw[: thd.azimuth_group_rank()]), sw[thd.azimuth_group_rank()]
        q = q[h0:h0 + hl, w0:w0 + wl].contiguous()
        H, W = q.shape
        self.register_buffer("quad_weight", q.float().reshape(1, 1, H, W), persistent=False)

    def _reduce(self, quad):
        if self.distributed:
            from . import distributed as thd
            quad = thd.reduce_from_spatial_region(quad.contiguous())
        return quad

    @torch.compiler.disable(recursive=True)
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._reduce(QuadLpFn.apply(x, None, None, self.quad_weight, 0, 1.0).to(x.dtype))

    def lp(self, a, b, wgt, p):
        """quadrature of |a - b|^p * wgt without materialising the integrand (b None = 0)."""
        return self._reduce(QuadLpFn.apply(a, b, wgt, self.quad_weight, 1, p))


def compute_spherical_bandlimit(img_shape, grid_type):
    """``makani/utils/grids.py:43-55``."""
    if grid_type == "equiangular":
        return min((img_shape[0] - 1) // 2, img_shape[1] // 2)
    if grid_type == "legendre-gauss":
        return min(img_shape[0] - 1, img_shape[1] // 2)
    raise NotImplementedError(f"Unknown type {grid_type} not implemented")


class SpecLpFn(torch.autograd.Function):
    """out[row] = sum_{l >= m} w(m) |c_lm|^p (* wgt) over an S-layout tensor (L, M, 2, R)."""

    @staticmethod
    def forward(ctx, S, wgt, p, w0, w1, tri_off, m_off):
        S = S.contiguous()
        L, M, _, R = S.shape
        nb = lib().mk_spec_lp_blocks(L, M)
        partial = torch.empty((nb, R), dtype=torch.float32, device=S.device)
        check(lib().mk_spec_lp_fwd(ptr(S), ptr(wgt) if wgt is not None else None, ptr(partial), L, M, R, tri_off, m_off,
                                   float(p), float(w0), float(w1), stream()), "mk_spec_lp_fwd")
        ctx.save_for_backward(S, wgt)
        ctx.meta = (float(p), float(w0), float(w1), tri_off, m_off)
        return partial.sum(0)

    @staticmethod
    def backward(ctx, g):
        S, wgt = ctx.saved_tensors
        p, w0, w1, tri_off, m_off = ctx.meta
        L, M, _, R = S.shape
        dS = torch.empty_like(S)
        g = g.contiguous().float()
        check(lib().mk_spec_lp_bwd(ptr(S), ptr(wgt) if wgt is not None else None, ptr(g), ptr(dS), L, M, R, tri_off, m_off,
                                   p, w0, w1, stream()), "mk_spec_lp_bwd")
        return dS, None, None, None, None, None, None


class SpectralLpLoss(nn.Module):
    """Computes the Lp loss in spectral (SH coefficient) space (``lp_loss.py:110-259``, base class
    ``base_loss.py:345-404``): SHT of the difference on the HIP path, then ONE kernel for
    ``|c|^p``, the Parseval weights (m = 0 once, m > 0 twice, 1/4pi) and the sum over (l, m) — on the SHT's
    internal layout, without materialising complex coefficients."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, p: Optional[float] = 2.0, relative: Optional[bool] = False,
                 squared: Optional[bool] = False, spatial_distributed: Optional[bool] = False,
                 eps: Optional[float] = 1.0e-6, lmax: Optional[int] = None, **kwargs):
        super().__init__()
        from . import distributed as thd
        from .sht import RealSHT
        self.img_shape, self.crop_shape, self.crop_offset = img_shape, crop_shape, crop_offset
        self.channel_names = channel_names
        self.spatial_distributed = bool(spatial_distributed) and thd.ensure_initialized()
        bandlimit = compute_spherical_bandlimit(img_shape, grid_type)
        if lmax is None or lmax > bandlimit:
            lmax = bandlimit
        if self.spatial_distributed:
            self.sht = thd.DistributedRealSHT(*img_shape, lmax=lmax, mmax=lmax, grid=grid_type)
            self._l_off, self._m_off = self.sht.l_off, self.sht.m_off
            l_loc = self.sht.l_shapes[self.sht.comm_rank_polar]
            m_loc = self.sht.m_shapes[self.sht.comm_rank_azimuth]
        else:
            self.sht = RealSHT(*img_shape, lmax=lmax, mmax=lmax, grid=grid_type).float()
            self._l_off = self._m_off = 0
            l_loc, m_loc = self.sht.lmax, self.sht.mmax
        m_weights = 2 * torch.ones(self.sht.mmax, dtype=torch.float32)
        m_weights[0] = 1.0
        m_weights = m_weights / (4.0 * math.pi)
        lm = torch.ones(self.sht.lmax, dtype=torch.float32)[:, None] * m_weights[None, :]
        lm = lm[self._l_off:self._l_off + l_loc, self._m_off:self._m_off + m_loc].contiguous()
        self.register_buffer("lm_weights", lm, persistent=False)
        self.p, self.relative, self.squared, self.eps = p, relative, squared, eps

    @property
    def type(self):
        return "deterministic"                                                  # LossType.Deterministic

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)

    @property
    def n_channels(self):
        return len(self.channel_names)

    def _s_weights(self, wgt, B, C, L, M, R, device):
        """broadcastable (B, C, L, M) weights -> (L, M, R) in the S-layout's row order"""
        if wgt is None:
            return None
        w = wgt.to(device=device, dtype=torch.float32).expand(B, C, L, M)
        Cp = R // B
        out = torch.zeros((L, M, B, Cp), dtype=torch.float32, device=device)
        out[:, :, :, :C] = w.permute(2, 3, 0, 1)
        return out.view(L, M, R)

    def _norm_p(self, x, wgt, w0, w1):
        """sum_{l,m} w(m) |sht(x)|^p per (b, c)"""
        if x.dim() != 4:
            raise ValueError(f"expected (B, C, H, W), got {tuple(x.shape)}")
        need_gpu(x)
        B, C = x.shape[:2]
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        S = self.sht.analysis(x.contiguous())
        L, M, _, R = S.shape
        w3 = self._s_weights(wgt, B, C, L, M, R, x.device)
        rows = SpecLpFn.apply(S, w3, self.p, w0, w1, self._l_off - self._m_off, self._m_off)
        out = rows.view(B, R // B)[:, :C]
        if self.spatial_distributed:
            from . import distributed as thd
            out = thd.reduce_from_spatial_region(out.contiguous())
        return out

    def abs(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None):
        inv_area = 1.0 / (4.0 * math.pi)
        normp = self._norm_p(prd - tar, wgt, inv_area, 2.0 * inv_area)
        return normp if self.squared else normp.pow(1.0 / self.p)

    def rel(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None):
        normp = self._norm_p(prd - tar, wgt, 1.0, 2.0)
        tar_normp = self._norm_p(tar, wgt, 1.0, 2.0)
        if not self.squared:
            normp, tar_normp = normp.pow(1.0 / self.p), tar_normp.pow(1.0 / self.p)
        return normp / (tar_normp + self.eps)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None, **kwargs):
        return self.rel(prd, tar, wgt) if self.relative else self.abs(prd, tar, wgt)


class SpectralH1Loss(SpectralLpLoss):
    """H1 seminorm loss on the sphere (``makani/utils/losses/h1_loss.py:30-180``): the p = 2 spectral loss with every
    degree weighted by l (l + 1).  Same kernels as ``SpectralLpLoss``; the degree weights ride in its weight operand."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, relative: Optional[bool] = False,
                 squared: Optional[bool] = False, spatial_distributed: Optional[bool] = False,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, p=2.0, relative=relative,
                         squared=squared, spatial_distributed=spatial_distributed, eps=eps)
        l = torch.arange(self.sht.lmax).float()
        h1 = (l * (l + 1))[self._l_off:self._l_off + self.lm_weights.shape[0]]
        self.register_buffer("h1_weights", h1.reshape(1, 1, -1), persistent=False)

    def _norm_p(self, x, wgt, w0, w1):
        h1 = self.h1_weights.reshape(1, 1, -1, 1)
        return super()._norm_p(x, h1 if wgt is None else wgt * h1, w0, w1)

    def abs(self, prd, tar, wgt=None):
        inv_area = 1.0 / (4.0 * math.pi)
        n2 = self._norm_p(prd - tar, wgt, inv_area, 2.0 * inv_area)
        return n2 if self.squared else torch.sqrt(n2)

    def rel(self, prd, tar, wgt=None):
        n2 = self._norm_p(prd - tar, wgt, 1.0, 2.0)
        t2 = self._norm_p(tar, wgt, 1.0, 2.0)
        if not self.squared:
            n2, t2 = torch.sqrt(n2), torch.sqrt(t2)
        return n2 / (t2 + self.eps)


class GeometricLpLoss(nn.Module):
    """Computes the Lp loss on the sphere (``lp_loss.py:28-107``)."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], p: Optional[float] = 2.0, relative: Optional[bool] = False,
                 squared: Optional[bool] = False, jacobian: Optional[str] = "s2",
                 grid_type: Optional[str] = "equiangular", spatial_distributed: Optional[bool] = False,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__()
        self.img_shape, self.crop_shape, self.crop_offset = img_shape, crop_shape, crop_offset
        self.channel_names = channel_names
        self.quadrature = GridQuadrature(grid_to_quadrature_rule(grid_type), img_shape=img_shape, crop_shape=crop_shape,
                                         crop_offset=crop_offset, normalize=True, distributed=spatial_distributed)
        self.spatial_distributed = self.quadrature.distributed
        self.p, self.relative, self.squared, self.eps = p, relative, squared, eps

    @property
    def type(self):
        return "deterministic"                                                  # LossType.Deterministic

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)

    @property
    def n_channels(self):
        return len(self.channel_names)

    def abs(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None):
        n = prd.shape[0]
        norms = self.quadrature.lp(prd, tar, wgt, self.p).reshape(n, -1)
        if not self.squared:
            norms = norms.pow(1.0 / self.p)
        return norms

    def rel(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None):
        n = prd.shape[0]
        diff = self.quadrature.lp(prd, tar, wgt, self.p).reshape(n, -1)
        tarn = self.quadrature.lp(tar, None, wgt, self.p).reshape(n, -1)
        norms = diff / (tarn + self.eps)
        if not self.squared:
            norms = norms.pow(1.0 / self.p)
        return norms

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None, **kwargs):
        return self.rel(prd, tar, wgt) if self.relative else self.abs(prd, tar, wgt)


# --------------------------------------------------------------------------- #
# ensemble CRPS (makani/utils/losses/crps_loss.py:277-452)
# --------------------------------------------------------------------------- #
_CRPS_TYPES = {"skillspread": 0, "probability weighted moment": 1, "naive skillspread": 2, "gauss": 3, "cdf": 4}


class CrpsFn(torch.autograd.Function):
    """out[b, c] = sum_p q[p] * w[b, c, p] * crps(obs[b, c, p], forecasts[b, :, c, p]); gradient w.r.t. the forecasts"""

    @staticmethod
    def forward(ctx, forecasts, obs, q, wgt, ctype, alpha, eps, ens_w=None):
        B, E, Cc, H, W = forecasts.shape
        ensemble_size_check(E, "CRPS")
        hw = H * W
        f, o = prep(forecasts), prep(obs)
        w = wgt.float().contiguous() if wgt is not None else None
        ch = lib().mk_crps_chunks(hw)
        partial = torch.empty((B * Cc, ch), dtype=torch.float32, device=f.device)
        check(lib().mk_crps(ptr(f), dtype_code(f), ptr(o), dtype_code(o), ptr(q), ptr(w), None, ptr(partial), None, B, E, Cc, hw,
                            ctype, float(alpha), float(eps), 0, ptr(ens_w), stream()), "mk_crps")
        ctx.save_for_backward(f, o, q, w if w is not None else torch.empty(0, device=f.device))
        ctx.meta = (ctype, alpha, eps, w is not None, forecasts.dtype)
        ctx.ens_w = ens_w
        return partial.sum(dim=1).reshape(B, Cc)

    @staticmethod
    def backward(ctx, g):
        f, o, q, w = ctx.saved_tensors
        ctype, alpha, eps, has_w, dt = ctx.meta
        B, E, Cc, H, W = f.shape
        gf = torch.empty_like(f)
        go = g.float().contiguous()
        check(lib().mk_crps(ptr(f), dtype_code(f), ptr(o), dtype_code(o), ptr(q), ptr(w) if has_w else None, ptr(go), None,
                            ptr(gf), B, E, Cc, H * W, ctype, float(alpha), float(eps), 1, ptr(ctx.ens_w), stream()), "mk_crps")
        return gf.to(dt), None, None, None, None, None, None, None


class CrpsComplexFn(torch.autograd.Function):
    """the "naive skillspread" score of COMPLEX members (``mk_crps_complex``): forecasts (B, E, C, L, M) complex64,
    obs (B, C, L, M) complex64 -> (B, C); gradient with respect to the forecasts"""

    @staticmethod
    def forward(ctx, forecasts, obs, q, wgt, alpha):
        B, E, Cc, H, W = forecasts.shape
        ensemble_size_check(E, "CRPS")
        hw = H * W
        f = torch.view_as_real(forecasts.to(torch.complex64).contiguous())
        o = torch.view_as_real(obs.to(torch.complex64).contiguous())
        w = wgt.float().contiguous() if wgt is not None else None
        ch = lib().mk_crps_chunks(hw)
        partial = torch.empty((B * Cc, ch), dtype=torch.float32, device=f.device)
        check(lib().mk_crps_complex(ptr(f), ptr(o), ptr(q), ptr(w), None, ptr(partial), None, B, E, Cc, hw, float(alpha), 0, stream()),
              "mk_crps_complex")
        ctx.save_for_backward(f, o, q, w if w is not None else torch.empty(0, device=f.device))
        ctx.meta = (alpha, w is not None)
        return partial.sum(dim=1).reshape(B, Cc)

    @staticmethod
    def backward(ctx, g):
        f, o, q, w = ctx.saved_tensors
        alpha, has_w = ctx.meta
        B, E, Cc, H, W, _ = f.shape
        gf = torch.empty_like(f)
        go = g.float().contiguous()
        check(lib().mk_crps_complex(ptr(f), ptr(o), ptr(q), ptr(w) if has_w else None, ptr(go), None, ptr(gf), B, E, Cc, H * W,
                                    float(alpha), 1, stream()), "mk_crps_complex")
        return torch.view_as_complex(gf), None, None, None, None


def _check_finite_weights(w):
    """Non-finite ``ensemble_weights`` are rejected at construction.  Deviation from the reference, stated: its kernels fold
    ``isnan(weights)`` into their NaN mask (``crps_loss.py:66-73,176-177``), so a NaN weight — one entry per member, broadcast
    over every grid point — silently zeroes the whole score (PWM) or drops the member everywhere (cdf); here that is an error."""
    if w is not None and not bool(torch.isfinite(w).all()):
        raise ValueError("ensemble_weights must be finite (the reference would mask every grid point of a member with a NaN weight)")


def _ens_w(w, E, crps_type="cdf"):
    if w is not None and w.numel() != E:
        raise ValueError(f"ensemble_weights holds {w.numel()} entries for an ensemble of {E}")
    return w if crps_type == "cdf" else None          # only the cdf kernel reads the values (PWM accepts and ignores them)


class _EnsembleLoss(nn.Module):
    """What the ensemble losses on the grid share (``GeometricBaseLoss`` of ``base_loss.py:261-342`` as the reference's use
    it): the quadrature of the (local) grid, the loss type, the channel count and weighting, the input checks, and the way
    from (B, E, C, H, W) members to the operands of a kernel over N points."""

    def __init__(self, img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed):
        super().__init__()
        self.img_shape, self.crop_shape, self.crop_offset = img_shape, crop_shape, crop_offset
        self.channel_names = channel_names
        self.quadrature = GridQuadrature(grid_to_quadrature_rule(grid_type), img_shape=img_shape, crop_shape=crop_shape,
                                         crop_offset=crop_offset, normalize=True, distributed=spatial_distributed)
        self.spatial_distributed = self.quadrature.distributed
        self.ensemble_distributed = ensemble_active(ensemble_distributed)                 # crps_loss.py:305-307
        # (the whole plane's weights: the ensemble-parallel path takes this rank's share of the points in forward)
        self.register_buffer("quad_weight_split", self.quadrature.quad_weight.reshape(1, 1, -1).contiguous(), persistent=False)

    @property
    def type(self):
        return "probabilistic"                                                  # LossType.Probabilistic

    @property
    def n_channels(self):
        return len(self.channel_names)

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)

    @staticmethod
    def _check(forecasts, observations, spatial_weights):
        check_forecast_dims(forecasts)
        check_weight_dims(spatial_weights, observations)

    def _points(self, forecasts, observations, spatial_weights):
        """forecasts (B, E, C, H, W), observations (B, C, H, W), weights broadcastable to them or None -> f (B, E, C, N),
        o (B, C, N), q (N), w (B, C, N) | None and ``sum_groups``, the process groups over which what the kernel sums over its
        N points has to be added: the ensemble group (members <-> a share of the points) before the spatial group."""
        f, o, q, w, group = flatten_and_split(forecasts, observations, self.quad_weight_split.reshape(-1), spatial_weights,
                                              self.ensemble_distributed)
        groups = [] if group is None else [group]
        if self.spatial_distributed:
            from . import distributed as thd
            groups.append(thd.spatial_group())
        return f, o, q, w, groups

    @staticmethod
    def _sum_shares(score, sum_groups):
        for group in sum_groups:
            score = ReduceFromGroupFn.apply(score, group)
        return score


class CRPSLoss(_EnsembleLoss):
    """``CRPSLoss`` of ``makani/utils/losses/crps_loss.py:277-452``: ``forward(forecasts (B, E, C, H, W), observations
    (B, C, H, W), spatial_weights=None) -> (B, C)``, the quadrature-weighted ensemble CRPS.  Score and quadrature are one HIP
    kernel (``csrc/crps.hip``), the gradient with respect to the forecasts one more.  Built: ``crps_type`` "skillspread"
    (default, with the almost-fair factor ``alpha``), "naive skillspread", "probability weighted moment", "gauss" and "cdf"
    (:55-122, with optional per-member ``ensemble_weights``; the "probability weighted moment" form accepts them too and, like the reference's kernel, ignores their values — finite values: non-finite weights raise, see ``_check_finite_weights``); any ensemble
    size 2..32; ``ensemble_distributed=True`` with a split "ensemble" group (``makani_amd.comm.init(h, w, ensemble=n)`` or
    makani's own tree) trades the members for a share of the grid points before scoring, as the reference does."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, crps_type: str = "skillspread",
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False,
                 ensemble_weights: Optional[torch.Tensor] = None, alpha: Optional[float] = 1.0, eps: Optional[float] = 1.0e-6,
                 **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed)
        # the reference hands ensemble_weights to the "cdf" kernel (:392-396) and to the "probability weighted moment" kernel
        # (:404-409), which ignores their values: accepted for both (and ignored by the latter, as there); other forms raise
        if ensemble_weights is not None and crps_type not in ("cdf", "probability weighted moment"):
            raise NotImplementedError("currently only constant ensemble weights are supported")
        _check_finite_weights(ensemble_weights)
        if crps_type not in _CRPS_TYPES:
            raise ValueError(f"Unknown CRPS crps_type {crps_type}")
        if crps_type not in ("skillspread", "naive skillspread") and alpha < 1.0:
            raise NotImplementedError("The alpha parameter (almost fair CRPS factor) is only supported for the skillspread kernels.")
        self.crps_type, self.alpha, self.eps = crps_type, alpha, eps
        self.register_buffer("ensemble_weights", None if ensemble_weights is None else ensemble_weights.float().reshape(-1).contiguous(),
                             persistent=False)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        self._check(forecasts, observations, spatial_weights)
        B, E, Cc, H, W = forecasts.shape
        if E == 1 and not self.ensemble_distributed:            # |obs - forecast| under the quadrature (crps_loss.py:375-377)
            crps = self.quadrature.lp(forecasts.squeeze(1), observations, spatial_weights, 1.0).reshape(B, Cc)
            return crps
        # members spread over the ensemble group are traded for a share of the grid points (crps_loss.py:362-373); that share
        # is scored with all members and the shares are summed (:441-442)
        f, o, q, w, groups = self._points(forecasts, observations, spatial_weights)
        crps = CrpsFn.apply(f.unsqueeze(-1), o.unsqueeze(-1), q, w.unsqueeze(-1) if w is not None else None,
                            _CRPS_TYPES[self.crps_type], self.alpha, self.eps, _ens_w(self.ensemble_weights, f.shape[1], self.crps_type))
        return self._sum_shares(crps, groups)


def _sht_pair(sht, forecasts, observations):
    """the coefficients of members and observation as the spectral ensemble losses take them: fp32, autocast off, / sqrt(4 pi)"""
    with torch.autocast(device_type=forecasts.device.type, enabled=False):
        f = sht(forecasts.float()) / math.sqrt(4.0 * math.pi)
        o = sht(observations.float()) / math.sqrt(4.0 * math.pi)
    return f, o


class SpectralCRPSLoss(SpectralLpLoss):
    """``SpectralCRPSLoss`` of ``makani/utils/losses/crps_loss.py:454-637`` (registered as "ensemble_spectral_crps"): the
    ensemble CRPS of the ABSOLUTE VALUES of the spherical-harmonic coefficients, summed with the Parseval weights of
    ``SpectralBaseLoss`` (m = 0 once, m > 0 twice, 1 / 4 pi).  ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W),
    spectral_weights=None) -> (B, C)``.  The transforms are the HIP SHT (fp32, autocast off, as the reference), the per-(l, m)
    ensemble score and its weighted sum the HIP kernel of ``CRPSLoss`` (``csrc/crps.hip``) with the (l, m) plane in the place of
    the grid; ``absolute=False`` scores the complex coefficients themselves with the naive skill / spread kernel
    (``mk_crps_complex``); ``ensemble_distributed=True`` as in ``CRPSLoss`` (absolute values only)."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmax: Optional[int] = None, crps_type: str = "skillspread",
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False,
                 ensemble_weights: Optional[torch.Tensor] = None, absolute: Optional[bool] = True, alpha: Optional[float] = 1.0,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed=spatial_distributed,
                         lmax=lmax)
        self.ensemble_distributed = ensemble_active(ensemble_distributed)
        if ensemble_weights is not None and crps_type != "cdf":
            raise NotImplementedError("currently only constant ensemble weights are supported")
        _check_finite_weights(ensemble_weights)
        if crps_type not in ("cdf", "skillspread", "probability weighted moment", "gauss"):     # what the reference's forward knows
            raise ValueError(f"Unknown CRPS crps_type {crps_type}")
        if crps_type not in ("skillspread", "naive skillspread") and alpha < 1.0:
            raise NotImplementedError("The alpha parameter (almost fair CRPS factor) is only supported for the skillspread kernels.")
        if not absolute and crps_type != "skillspread":              # crps_loss.py:540-545
            raise ValueError(f"the non-absolute path only works with the naive 'skillspread' CRPS kernel, but got crps_type {crps_type}")
        self.crps_type, self.alpha, self.eps, self.absolute = crps_type, alpha, eps, absolute
        self.register_buffer("ensemble_weights", None if ensemble_weights is None else ensemble_weights.float().reshape(-1).contiguous(),
                             persistent=False)

    @property
    def type(self):
        return "probabilistic"                                                  # LossType.Probabilistic

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spectral_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        from . import distributed as thd
        check_forecast_dims(forecasts)
        check_weight_dims(spectral_weights, observations, found=False)
        dtype = forecasts.dtype
        f, o = _sht_pair(self.sht, forecasts, observations)
        if self.absolute:
            f, o = torch.abs(f).to(dtype), torch.abs(o).to(dtype)
        B, E, Cc, L, M = f.shape
        if self.ensemble_distributed:            # crps_loss.py:566-581: members <-> (l, m) points over the ensemble group
            if not self.absolute:
                raise NotImplementedError("the ensemble-parallel spectral CRPS is built for absolute=True")
            w = (spectral_weights.expand(B, Cc, L, M).reshape(B, Cc, L * M) if spectral_weights is not None else None)
            fe, oe, qe, we, group = ensemble_split(f.reshape(B, E, Cc, L * M), o.reshape(B, Cc, L * M),
                                                    self.lm_weights.reshape(-1).contiguous(), w)
            crps = CrpsFn.apply(fe.unsqueeze(-1), oe.unsqueeze(-1), qe, we.unsqueeze(-1) if we is not None else None,
                                _CRPS_TYPES[self.crps_type], self.alpha, self.eps, _ens_w(self.ensemble_weights, fe.shape[1]))
            crps = ReduceFromGroupFn.apply(crps, group)
            return thd.reduce_from_spatial_region(crps) if self.spatial_distributed else crps
        if not self.absolute and E > 1:        # the naive kernel on the complex coefficients themselves (crps_loss.py:605-608)
            w = spectral_weights.expand(B, Cc, L, M) if spectral_weights is not None else None
            crps = CrpsComplexFn.apply(f, o, self.lm_weights.reshape(-1).contiguous(), w, self.alpha)
            return thd.reduce_from_spatial_region(crps) if self.spatial_distributed else crps
        if E == 1:
            w = self.lm_weights if spectral_weights is None else spectral_weights * self.lm_weights
            crps = (torch.abs(o - f.squeeze(1)).float() * w).reshape(B, Cc, L * M).sum(dim=-1)
        else:
            w = spectral_weights.expand(B, Cc, L, M) if spectral_weights is not None else None
            crps = CrpsFn.apply(f.contiguous(), o.contiguous(), self.lm_weights.reshape(-1).contiguous(), w, _CRPS_TYPES[self.crps_type],
                                self.alpha, self.eps, _ens_w(self.ensemble_weights, E))
        if self.spatial_distributed:
            crps = thd.reduce_from_spatial_region(crps)
        return crps


# --------------------------------------------------------------------------- #
# ensemble CRPS of gradients and of the wind field's vorticity / divergence decomposition
# (makani/utils/losses/crps_loss.py:640-1019, base classes base_loss.py:427-585)
# --------------------------------------------------------------------------- #
def get_wind_channels(channel_names):
    """``makani/utils/features.py:83-94``: every ``uX`` with a ``vX`` in the list gives the index pair (u, v)"""
    out = []
    for c, ch in enumerate(channel_names):
        if ch[0] == "u" and ("v" + ch[1:]) in channel_names:
            out += [c, channel_names.index("v" + ch[1:])]
    return out


_SURFACE_01 = ("u10m", "v10m", "u100m", "v100m", "tp", "sp", "msl", "tcwv", "sst")


_HANDLER_WEIGHTS = False          # True while LossHandler asks a loss for its weights (``_handler_weights``)


@contextlib.contextmanager
def _handler_weights():
    """Inside, ``channel_weighting`` returns what the reference's helper returns: the weights divided by their sum and multiplied
    by the time-difference scale.  Outside (a loss asked directly) the weights stay as this project has always returned them:
    not normalised, a time-difference scale an error."""
    global _HANDLER_WEIGHTS
    before, _HANDLER_WEIGHTS = _HANDLER_WEIGHTS, True
    try:
        yield
    finally:
        _HANDLER_WEIGHTS = before


def channel_weighting(channel_names, channel_weight_type, time_diff_scale=None):
    """the "constant", "auto" and "new auto" rules of ``base_loss.py:33-72`` (pressure-level channels weighted by their level);
    the tabulated "custom" weights and the time-difference scalings are not carried here"""
    w = torch.ones(len(channel_names), dtype=torch.float32)
    if channel_weight_type in ("auto", "new auto"):
        new = channel_weight_type == "new auto"
        for c, chn in enumerate(channel_names):
            if chn in _SURFACE_01:
                w[c] = 0.1
            elif chn in ("t2m", "2d"):
                w[c] = 2.0 if new else 1.0
            elif chn[0] in "zuvtrq":
                w[c] = max(0.3, 0.001 * float(chn[1:])) if new else 0.001 * float(chn[1:])
            else:
                w[c] = 0.01
    elif channel_weight_type != "constant":
        raise NotImplementedError(f"channel weighting {channel_weight_type!r} is not built on the HIP path (constant, auto, new auto)")
    if _HANDLER_WEIGHTS:          # LossHandler asks: normalised, times the time-difference scale (base_loss.py:233-240)
        w = w / torch.sum(w)
        return w if time_diff_scale is None else w * time_diff_scale
    if time_diff_scale is not None:
        raise NotImplementedError("time-difference scaling of the channel weights is not built on the HIP path")
    return w


class _EnsembleGridLoss(_EnsembleLoss):
    """what ``GradientCRPSLoss`` and ``VortDivCRPSLoss`` share: constructor checks, quadrature, the score on the grid"""

    def __init__(self, img_shape, crop_shape, crop_offset, channel_names, grid_type, crps_type, spatial_distributed,
                 ensemble_distributed, ensemble_weights, alpha, eps):
        if spatial_distributed or ensemble_distributed:
            import torch.distributed as dist
            from . import comm as _comm
            _comm.autodetect()
            split = (spatial_distributed and _comm.is_distributed("spatial") and _comm.get_size("spatial") > 1) or \
                (ensemble_distributed and _comm.is_distributed("ensemble") and _comm.get_size("ensemble") > 1)
            if split and not (dist.is_available() and dist.is_initialized()):
                raise NotImplementedError(f"{type(self).__name__}: spatial_distributed / ensemble_distributed with a group larger than "
                                          "one needs an initialised torch.distributed process group in this process (the distributed "
                                          "vector transforms and the ensemble exchange run over it)")
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed)
        if tuple(crop_shape) != tuple(img_shape):
            raise NotImplementedError("the vector-transform losses score the whole sphere (crop_shape == img_shape)")
        if crps_type not in ("skillspread", "naive skillspread") and alpha < 1.0:
            raise NotImplementedError("The alpha parameter (almost fair CRPS factor) is only supported for the skillspread kernels.")
        if ensemble_weights is not None and crps_type != "cdf":            # crps_loss.py:810-811 (the gauss branch cannot run there)
            raise NotImplementedError("currently only constant ensemble weights are supported")
        _check_finite_weights(ensemble_weights)
        self.crps_type, self.alpha, self.eps = crps_type, alpha, eps
        self.register_buffer("ensemble_weights", None if ensemble_weights is None else ensemble_weights.float().reshape(-1).contiguous(),
                             persistent=False)

    @staticmethod
    def _check(forecasts, observations, spatial_weights):
        _EnsembleLoss._check(forecasts, observations, spatial_weights)
        need_gpu(forecasts)

    def _score(self, forecasts, observations, spatial_weights):
        """forecasts (B, E, C, H, W), observations (B, C, H, W) -> (B, C), as ``CRPSLoss.forward``"""
        if self.crps_type not in ("cdf", "skillspread", "gauss"):              # what the reference's forward knows
            raise ValueError(f"Unknown CRPS crps_type {self.crps_type}")
        B, E, Cc, H, W = forecasts.shape
        if E == 1 and not self.ensemble_distributed:              # (the quadrature sums over the spatial group itself)
            return self.quadrature.lp(forecasts.squeeze(1), observations, spatial_weights, 1.0).reshape(B, Cc)
        if self.spatial_distributed or self.ensemble_distributed:
            # the score stage of CRPSLoss on this rank's points with the local quadrature weights: members <-> a share of the
            # points over the ensemble group, then the SUM over the ensemble and the spatial group (crps_loss.py:775-841)
            f, o, q, w, groups = self._points(forecasts, observations, spatial_weights)
            crps = CrpsFn.apply(f.unsqueeze(-1), o.unsqueeze(-1), q, w.unsqueeze(-1) if w is not None else None,
                                _CRPS_TYPES[self.crps_type], self.alpha, self.eps, _ens_w(self.ensemble_weights, f.shape[1], self.crps_type))
            return self._sum_shares(crps, groups)
        w = spatial_weights.expand(B, Cc, H, W) if spatial_weights is not None else None
        return CrpsFn.apply(forecasts, observations, self.quad_weight_split.reshape(-1), w, _CRPS_TYPES[self.crps_type], self.alpha,
                            self.eps, _ens_w(self.ensemble_weights, E, self.crps_type))

    def _transforms(self, lmax, grid_type, forward_vector):
        """(forward transform, inverse vector transform) on the whole sphere, or on this rank's shard of it"""
        nlat, nlon = self.img_shape
        kw = dict(lmax=lmax, mmax=lmax, grid=grid_type)
        if self.spatial_distributed:
            from . import distributed as thd
            fw = (thd.DistributedRealVectorSHT if forward_vector else thd.DistributedRealSHT)(nlat, nlon, **kw)
            return fw, thd.DistributedInverseRealVectorSHT(fw.nlat, fw.nlon, **kw)
        from .sht import RealSHT, RealVectorSHT, InverseRealVectorSHT
        fw = (RealVectorSHT if forward_vector else RealSHT)(nlat, nlon, **kw)
        return fw, InverseRealVectorSHT(fw.nlat, fw.nlon, **kw)


class GradientCRPSLoss(_EnsembleGridLoss):
    """``GradientCRPSLoss`` of ``makani/utils/losses/crps_loss.py:640-844`` ("ensemble_gradient_crps"): the ensemble CRPS of the
    surface gradient of every channel — ``absolute=True``: of its magnitude, (B, C); ``False``: of both components, (B, 2 C) in
    the order (c, component).  Scalar analysis (HIP SHT), then the vector synthesis with a ZERO toroidal part
    (``InverseRealVectorSHT.synthesis(t_zero=True)``: nothing is stored or multiplied for it), in fp32 whatever the autocast
    state; score and quadrature are the kernels of ``CRPSLoss``.  ``spatial_distributed`` / ``ensemble_distributed`` as in
    ``CRPSLoss``: the transforms are the distributed pair on this rank's shard of the sphere and this rank's members."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmax: Optional[int] = None, crps_type: str = "skillspread",
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False,
                 ensemble_weights: Optional[torch.Tensor] = None, absolute: Optional[bool] = True, alpha: Optional[float] = 1.0,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, crps_type, spatial_distributed,
                         ensemble_distributed, ensemble_weights, alpha, eps)
        self.absolute = absolute
        self.sht, self.ivsht = self._transforms(lmax, grid_type, False)

    @property
    def n_channels(self):
        return len(self.channel_names) * (1 if self.absolute else 2)

    @staticmethod
    def expand_channel_weights(chw):
        return [w for w in chw for _ in range(2)]

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None):
        chw = channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)
        return chw if self.absolute else self.expand_channel_weights(chw)

    def _gradient(self, x, dtype):
        """(N, C, H, W) -> (N, C, H, W) |grad| or (N, 2 C, H, W) components, in ``dtype``"""
        from . import ops
        N, Cc, H, W = x.shape
        S = self.sht.analysis(x.float().contiguous())                               # (L, M, 2, N * Cp), rows (n, c)
        Cp = S.shape[-1] // N
        P = N * Cp
        Rp = ops.round32(P)
        if Rp != P:                                                                 # the vector kernel's rows come in 32s
            S = torch.nn.functional.pad(S, (0, Rp - P))
        g = self.ivsht.synthesis(S, P, t_zero=True).to(dtype)                       # (2, N * Cp, H, W)
        g = g.view(2, N, Cp, H, W)[:, :, :Cc]
        if self.absolute:
            return g.pow(2).sum(dim=0).sqrt()
        return g.permute(1, 2, 0, 3, 4).reshape(N, 2 * Cc, H, W)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        self._check(forecasts, observations, spatial_weights)
        B, E, Cc, H, W = forecasts.shape
        dtype = forecasts.dtype
        with torch.autocast(device_type=forecasts.device.type, enabled=False):
            f = self._gradient(forecasts.reshape(B * E, Cc, H, W), dtype)
            o = self._gradient(observations, dtype)
        Co = f.shape[1]
        return self._score(f.reshape(B, E, Co, H, W).contiguous(), o.contiguous(), spatial_weights)


class VortDivCRPSLoss(_EnsembleGridLoss):
    """``VortDivCRPSLoss`` of ``makani/utils/losses/crps_loss.py:847-1019`` ("ensemble_vort_div_crps"): every (u, v) pair of the
    channel list goes through the vector transform round trip (fp32, autocast off) and is scattered back, the other channels
    pass through; the ensemble CRPS of the result, (B, C).  Analysis and synthesis are chained on the internal S layout (no
    complex64 tensor in between).  ``spatial_distributed`` / ``ensemble_distributed`` as in ``CRPSLoss``; on a split sphere the round trip
    hands the Legendre-phase operand from the analysis to the synthesis and skips both polar exchanges."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, crps_type: str = "skillspread",
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False,
                 ensemble_weights: Optional[torch.Tensor] = None, alpha: Optional[float] = 1.0, eps: Optional[float] = 1.0e-6,
                 lmax: Optional[int] = None, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, crps_type, spatial_distributed,
                         ensemble_distributed, ensemble_weights, alpha, eps)
        self.register_buffer("wind_chans", torch.LongTensor(get_wind_channels(channel_names)), persistent=False)
        self.vsht, self.isht = self._transforms(lmax, grid_type, True)

    def average_wind_weights(self, chw):
        wind = self.wind_chans.to(chw.device)
        u, v = wind[0::2], wind[1::2]
        avg = (chw[u] + chw[v]) / 2
        chw[u] = avg
        chw[v] = avg
        return chw

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        return self.average_wind_weights(channel_weighting(self.channel_names, channel_weight_type, time_diff_scale))

    def _round_trip(self, x):
        """(N, C, H, W) fp32 -> the same with the wind channels replaced by their transform round trip"""
        Cw = self.wind_chans.shape[0]
        if Cw == 0:
            return x
        N, Cc, H, W = x.shape
        wind = x[:, self.wind_chans].reshape(N * (Cw // 2), 2, H, W)
        xc = wind.transpose(0, 1).contiguous()                                      # (2, P, H, W): component outermost
        if self.spatial_distributed:            # the l <-> pairs exchange of the analysis and its mirror in the synthesis cancel
            S = self.vsht.analysis(xc, legendre_phase=True)
            back = self.isht.synthesis(S, xc.shape[1], legendre_phase=True)
        else:
            S = self.vsht.analysis(xc)
            back = self.isht.synthesis(S, xc.shape[1])                              # (2, P, H, W)
        back = back.transpose(0, 1).reshape(N, Cw, H, W)
        return x.index_copy(1, self.wind_chans, back)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        self._check(forecasts, observations, spatial_weights)
        B, E, Cc, H, W = forecasts.shape
        with torch.autocast(device_type=forecasts.device.type, enabled=False):
            f = self._round_trip(forecasts.float().reshape(B * E, Cc, H, W)).reshape(B, E, Cc, H, W)
            o = self._round_trip(observations.float())
        return self._score(f.contiguous(), o.contiguous(), spatial_weights)


# --------------------------------------------------------------------------- #
# ensemble energy scores (makani/utils/losses/energy_score.py:30-652)
# --------------------------------------------------------------------------- #
_ES_COMPLEX = 2            # `kind` of mk_escore_*: complex64 members (MK_F32 / MK_BF16 otherwise)


class EnergyScoreFn(torch.autograd.Function):
    """The three stages of ``csrc/escore.hip``.  forecasts (B, E, C, N) f32 | bf16 | complex64 in that layout, obs (B, C, N),
    q (N), wgt optional (B, C, N); the plane of N points is ``nseg`` segments.  ``mk_escore_sums`` -> sums (B, C, nseg, K);
    the sums are added over ``sum_groups`` (process groups: the all-reduces of the parallel variants fall BEFORE the root);
    ``finish(sums, loss, table, B, E, C, nseg, reduce, p)`` — ``_escore_finish`` or ``_mmd_finish`` with their scalars —
    -> loss (B, C_out) and the table d loss / d sums, kept for ``mk_escore_grad``.  Gradient with respect to the forecasts
    only (the backward of a SUM all-reduce is the identity)."""

    @staticmethod
    def forward(ctx, forecasts, obs, q, wgt, nseg, nanmode, reduce, p, finish, sum_groups):
        B, E, Cc, N = forecasts.shape
        if forecasts.is_complex():
            kind = _ES_COMPLEX
            f = torch.view_as_real(forecasts.to(torch.complex64).contiguous())
            o = torch.view_as_real(obs.to(torch.complex64).contiguous())
        else:
            f = prep(forecasts)
            kind = dtype_code(f)
            o = obs.float().contiguous()
        q = q.float().contiguous()
        w = wgt.float().contiguous() if wgt is not None else None
        K = E + E * (E - 1) // 2
        sums = torch.empty((B, Cc, nseg, K), dtype=torch.float32, device=f.device)
        nws = lib().mk_escore_sums_workspace(B, E, Cc, N, nseg, nanmode)
        ws = torch.empty((nws,), dtype=torch.float32, device=f.device) if nws else None
        check(lib().mk_escore_sums(ptr(f), kind, ptr(o), ptr(q), ptr(w), ptr(sums), ptr(ws), B, E, Cc, N, nseg, nanmode, float(p),
                                   stream()), "mk_escore_sums")
        from . import ops
        for group in sum_groups:
            ops._all_reduce_sum(sums, group)
        Cout = 1 if reduce else Cc
        loss = torch.empty((B, Cout), dtype=torch.float32, device=f.device)
        table = torch.empty((B, Cout, nseg, K), dtype=torch.float32, device=f.device)
        finish(sums, loss, table, B, E, Cc, nseg, reduce, p)
        ctx.save_for_backward(f, o, q, w if w is not None else torch.empty(0, device=f.device), table)
        ctx.meta = (kind, w is not None, nseg, nanmode, float(p), forecasts.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        f, o, q, w, table = ctx.saved_tensors
        kind, has_w, nseg, nanmode, p, dt = ctx.meta
        B, E, Cc, N = f.shape[:4]
        gf = torch.empty_like(f)
        go = g.float().contiguous()
        check(lib().mk_escore_grad(ptr(f), kind, ptr(o), ptr(q), ptr(w) if has_w else None, ptr(table), ptr(go), ptr(gf), B, E, Cc,
                                   table.shape[1], N, nseg, nanmode, p, stream()), "mk_escore_grad")
        gf = torch.view_as_complex(gf) if kind == _ES_COMPLEX else gf.to(dt)
        return (gf,) + (None,) * 9


def _escore_finish(scale, beta, alpha, eps):
    """stage 2 of the energy scores (``mk_escore_finish``); ``scale`` (1 | C_out entries, or None) tempers the spread term"""
    def finish(sums, loss, table, B, E, Cc, nseg, reduce, p):
        sc = scale.float().contiguous() if scale is not None else None
        check(lib().mk_escore_finish(ptr(sums), ptr(sc), sc.numel() if sc is not None else 0, ptr(loss), ptr(table), B, E, Cc, nseg,
                                     int(reduce), float(p), float(beta), float(alpha), float(eps), stream()), "mk_escore_finish")
    return finish


def _escore_checks(forecasts, ensemble_weights):
    check_forecast_dims(forecasts)
    if ensemble_weights is not None:
        raise NotImplementedError("currently only constant ensemble weights are supported")


class _EnergyScoreMixin:
    """what ``channel_reduction`` changes: one output channel, with weight one"""

    @property
    def n_channels(self):
        return 1 if self.channel_reduction else len(self.channel_names)

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: str = None) -> torch.Tensor:
        if self.channel_reduction:
            return torch.ones(1)
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)


class LpEnergyScoreLoss(_EnergyScoreMixin, _EnsembleLoss):
    """``LpEnergyScoreLoss`` of ``makani/utils/losses/energy_score.py:30-250`` ("lp_energy_score"; "l2_energy_score" is the
    alias ``L2EnergyScoreLoss``): mean_e ||o - f_e||^beta - (E - 1 + alpha) / (E^2 (E - 1)) sum_{i<j} ||f_i - f_j||^beta with
    the quadrature-weighted Lebesgue norm ||x|| = (sum_n q w |x_n|^p)^(1/p) over the grid, per channel or (``channel_reduction``)
    over all channels.  ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W), spatial_weights=None,
    lead_time_step=None) -> (B, C) | (B, 1)``.  The members are read in place, once for E <= 8 (``csrc/escore.hip``); no pair
    tensor exists.  1 <= E <= 32 (more: NotImplementedError).

    Deviation, stated: ``p < 1`` raises NotImplementedError — the reference's autograd yields NaN gradients at coincident
    members there (|d|^(p - 1) at d = 0)."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, spatial_distributed: Optional[bool] = False,
                 ensemble_distributed: Optional[bool] = False, ensemble_weights: Optional[torch.Tensor] = None,
                 channel_reduction: Optional[bool] = True, alpha: Optional[float] = 1.0, beta: Optional[float] = 1.0,
                 p: Optional[float] = 2.0, eps: Optional[float] = 1.0e-6, spread_temper_steps: Optional[int] = 0, **kwargs):
        if float(p) < 1.0:
            raise NotImplementedError(f"p = {p}: the energy score is built for p >= 1 (the gradient of |d|^p is unbounded at "
                                      "coincident members for p < 1)")
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed)
        self.channel_reduction, self.alpha, self.beta, self.p, self.eps = channel_reduction, alpha, beta, float(p), eps
        self.spread_temper_steps = spread_temper_steps
        self.register_buffer("ensemble_weights", ensemble_weights, persistent=False)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                lead_time_step: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        _escore_checks(forecasts, self.ensemble_weights)
        check_weight_dims(spatial_weights, observations)
        need_gpu(forecasts)
        # members <-> a share of the points (:139-151), the sums added over the group (:188-190)
        f, o, q, w, groups = self._points(forecasts, observations, spatial_weights)
        ensemble_size_check(f.shape[1], "energy-score")
        scale = None
        if self.training and self.spread_temper_steps > 0 and lead_time_step is not None:       # :243-245
            scale = torch.clamp(lead_time_step.float().to(f.device) / self.spread_temper_steps, min=1.0).reshape(-1)
            if scale.numel() not in (1, self.n_channels):
                raise ValueError(f"lead_time_step holds {scale.numel()} entries for {self.n_channels} output channels")
        return EnergyScoreFn.apply(f, o, q, w, 1, 0, self.channel_reduction, self.p,
                                   _escore_finish(scale, self.beta, self.alpha, self.eps), groups)


L2EnergyScoreLoss = LpEnergyScoreLoss          # backward-compatibility alias, as the reference's


def _ensemble_split_lm(f, o, q):
    """f (B, E_loc, C, L, M) complex, o (B, C, L, M), q (L, M): the members of the group on this rank's share of the
    orders m (the reference's ``distributed_transpose(..., (-1, 0))`` of the last axis).  The exchange moves real tensors:
    (re, im) travel as two rows of the channel axis."""
    B, E, Cc, L, M = f.shape
    fr = torch.view_as_real(f.contiguous()).permute(0, 1, 2, 3, 5, 4).reshape(B, E, Cc * L * 2, M)
    fr, os_, qs, _, group = ensemble_split(fr, o, q, None)
    Ml = fr.shape[-1]
    fs = torch.view_as_complex(fr.reshape(B, -1, Cc, L, 2, Ml).permute(0, 1, 2, 3, 5, 4).contiguous())
    return fs, os_, qs, group


class _SpectralEnergyScore(_EnergyScoreMixin, SpectralLpLoss):
    """the spectral energy scores: HIP ``RealSHT`` of members and observation (fp32, autocast off, / sqrt(4 pi)), then the
    kernels of ``csrc/escore.hip`` on the complex coefficients (squared modulus; a coefficient where the observation or any
    member is NaN is masked)"""

    def __init__(self, img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed,
                 ensemble_distributed, ensemble_weights, channel_reduction, alpha, beta, eps):
        SpectralLpLoss.__init__(self, img_shape, crop_shape, crop_offset, channel_names, grid_type,
                                spatial_distributed=spatial_distributed, lmax=lmax, eps=eps)
        self.ensemble_distributed = ensemble_active(ensemble_distributed)
        self.channel_reduction, self.alpha, self.beta = channel_reduction, alpha, beta
        self.register_buffer("ensemble_weights", ensemble_weights, persistent=False)

    type = _EnsembleLoss.type                                                   # (the rest of that base belongs to the grid)

    _ensemble_split_lm = staticmethod(_ensemble_split_lm)          # (shared with the coherence losses below)

    @property
    def type(self):
        return "probabilistic"                                                  # LossType.Probabilistic

    def _score(self, forecasts, observations, per_degree):
        from . import comm as _comm
        _escore_checks(forecasts, self.ensemble_weights)
        need_gpu(forecasts)
        f, o = _sht_pair(self.sht, forecasts, observations)
        q = self.lm_weights
        groups = []
        if self.ensemble_distributed:
            f, o, q, group = self._ensemble_split_lm(f, o, q)
            groups.append(group)
        if self.spatial_distributed:                # per degree: the orders are summed over "w", the degrees (below) over "h"
            from . import distributed as thd
            if not per_degree:
                groups.append(thd.spatial_group())
            elif _comm.get_size("w") > 1:
                groups.append(_comm.get_group("w"))
        B, E, Cc, L, M = f.shape
        ensemble_size_check(E, "energy-score")
        loss = EnergyScoreFn.apply(f.reshape(B, E, Cc, L * M), o.reshape(B, Cc, L * M), q.reshape(-1), None, L if per_degree else 1, 1,
                                   self.channel_reduction, 2.0, _escore_finish(None, self.beta, self.alpha, self.eps), groups)
        if per_degree and self.spatial_distributed and _comm.get_size("h") > 1:
            loss = ReduceFromGroupFn.apply(loss, _comm.get_group("h"))
        return loss


class SobolevEnergyScoreLoss(_SpectralEnergyScore):
    """``SobolevEnergyScoreLoss`` of ``makani/utils/losses/energy_score.py:257-460`` ("sobolev_energy_score"): the energy score
    in the Sobolev norm ||x||^2 = sum_{l,m} (offset + relative_weight l (l + 1))^fraction w(m) |x_lm|^2 (w(0) = 1, w(m > 0) = 2)
    of the spherical-harmonic coefficients, per channel or over all channels.  ``forward(forecasts (B, E, C, H, W),
    observations (B, C, H, W)) -> (B, C) | (B, 1)``."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmax: Optional[int] = None, spatial_distributed: Optional[bool] = False,
                 ensemble_distributed: Optional[bool] = False, ensemble_weights: Optional[torch.Tensor] = None,
                 channel_reduction: Optional[bool] = True, alpha: Optional[float] = 1.0, beta: Optional[float] = 1.0,
                 offset: Optional[float] = 1.0, fraction: Optional[float] = 1.0, relative_weight: Optional[float] = 1.0,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed,
                         ensemble_distributed, ensemble_weights, channel_reduction, alpha, beta, eps)
        self.fraction, self.offset, self.relative_weight = fraction, offset, relative_weight
        l = torch.arange(self.sht.lmax, dtype=torch.float32)
        m_weights = 2 * torch.ones(self.sht.mmax, dtype=torch.float32)
        m_weights[0] = 1.0
        lm = (offset + relative_weight * l * (l + 1)).pow(fraction)[:, None] * m_weights[None, :]                 # :308-315
        Ll, Ml = self.lm_weights.shape
        self.register_buffer("lm_weights", lm[self._l_off:self._l_off + Ll, self._m_off:self._m_off + Ml].contiguous(), persistent=False)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, ensemble_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        return self._score(forecasts, observations, per_degree=False)


class SpectralL2EnergyScoreLoss(_SpectralEnergyScore):
    """``SpectralL2EnergyScoreLoss`` of ``makani/utils/losses/energy_score.py:463-652`` ("spectral_l2_energy_score"): one L2
    energy score per degree l (the norm sums the Parseval-weighted |x_lm|^2 over the orders m), summed over the degrees.
    ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W)) -> (B, C) | (B, 1)``."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmax: Optional[int] = None, spatial_distributed: Optional[bool] = False,
                 ensemble_distributed: Optional[bool] = False, ensemble_weights: Optional[torch.Tensor] = None,
                 channel_reduction: Optional[bool] = True, alpha: Optional[float] = 1.0, beta: Optional[float] = 1.0,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed,
                         ensemble_distributed, ensemble_weights, channel_reduction, alpha, beta, eps)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, ensemble_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        return self._score(forecasts, observations, per_degree=True)


# --------------------------------------------------------------------------- #
# adjusted MSE, ensemble likelihood, Gaussian MMD (makani/utils/losses/amse_loss.py, likelihood_loss.py, mmd_loss.py)
# --------------------------------------------------------------------------- #
class AmseSumsFn(torch.autograd.Function):
    """``csrc/amse.hip``: X, Y (B, C, L, M) complex64 and an optional weight (B, C, L, M) -> sums (B, C, L, 3): the Parseval
    sums over the orders of |x|^2, |y|^2 and Re(x conj y), with the 1 / 4 pi.  The backward reads X and Y once and writes both
    gradients (the target's only when it is asked for)."""

    @staticmethod
    def forward(ctx, X, Y, wgt, tri_off, m_off):
        B, Cc, L, M = X.shape
        x = torch.view_as_real(X.to(torch.complex64).contiguous())
        y = torch.view_as_real(Y.to(torch.complex64).contiguous())
        w = wgt.float().contiguous() if wgt is not None else None
        sums = torch.empty((B, Cc, L, 3), dtype=torch.float32, device=x.device)
        check(lib().mk_amse_sums(ptr(x), ptr(y), ptr(w), ptr(sums), B * Cc, L, M, tri_off, m_off, stream()), "mk_amse_sums")
        ctx.save_for_backward(x, y, w if w is not None else torch.empty(0, device=x.device))
        ctx.meta = (w is not None, tri_off, m_off)
        return sums

    @staticmethod
    def backward(ctx, g):
        x, y, w = ctx.saved_tensors
        has_w, tri_off, m_off = ctx.meta
        B, Cc, L, M = x.shape[:4]
        t = g.float().contiguous()
        dx = torch.empty_like(x)
        dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        check(lib().mk_amse_grad(ptr(x), ptr(y), ptr(w) if has_w else None, ptr(t), ptr(dx), ptr(dy), B * Cc, L, M, tri_off, m_off,
                                 stream()), "mk_amse_grad")
        return torch.view_as_complex(dx), (torch.view_as_complex(dy) if dy is not None else None), None, None, None


class SpectralAMSELoss(SpectralLpLoss):
    """``SpectralAMSELoss`` of ``makani/utils/losses/amse_loss.py:29-114`` ("amse", arXiv:2501.19374): per degree l the power of
    prediction and target and their coherence, ``(|x| - |y|)^2 + 2 max(|x|^2, |y|^2) (1 - coh)``, summed over l.
    ``forward(prd (B, C, H, W), tar (B, C, H, W), wgt=None) -> (B, C)``.  HIP SHT (fp32, autocast off), then ONE kernel for the
    three Parseval sums of a degree (``csrc/amse.hip``) and one for both gradients; the finish of :100-110 works on the
    (B, C, L, 3) sums in torch.  ``spatial_distributed``: the sums are added over the "w" group before the finish, the loss
    over the "h" group after it.  The sums are kept in fp32 whatever the input dtype; the result is cast to it."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, spatial_distributed: Optional[bool] = False,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed=spatial_distributed, eps=eps)

    @property
    def type(self):
        return "deterministic"                                                  # LossType.Deterministic

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        if prd.dim() != 4:
            raise ValueError(f"expected (B, C, H, W), got {tuple(prd.shape)}")
        need_gpu(prd)
        from . import comm as _comm
        ptype = prd.dtype
        with torch.autocast(device_type=prd.device.type, enabled=False):
            x = self.sht(prd.float())
            y = self.sht(tar.float())
        B, Cc, L, M = x.shape
        w = wgt.to(x.device).expand(B, Cc, L, M) if wgt is not None else None
        sums = AmseSumsFn.apply(x, y, w, self._l_off - self._m_off, self._m_off)
        if self.spatial_distributed and _comm.get_size("w") > 1:
            sums = ReduceFromGroupFn.apply(sums, _comm.get_group("w"))
        xnorm2, ynorm2, xycoh_sum = sums.unbind(-1)
        xnorm, ynorm = torch.sqrt(xnorm2), torch.sqrt(ynorm2)
        xycoh = xycoh_sum / torch.sqrt(xnorm2 * ynorm2 + self.eps)             # eps inside the root (:104)
        loss = torch.square(xnorm - ynorm) + 2 * torch.maximum(xnorm2, ynorm2) * (1 - xycoh)
        loss = torch.sum(loss, dim=-1)
        if self.spatial_distributed and _comm.get_size("h") > 1:
            loss = ReduceFromGroupFn.apply(loss, _comm.get_group("h"))
        return loss.to(ptype)


class EnsNllFn(torch.autograd.Function):
    """out[b, c] = sum_p q[p] * w[b, c, p] * nll(obs[b, c, p], forecasts[b, :, c, p]) (``csrc/ensnll.hip``); gradient with
    respect to the forecasts.  forecasts (B, E, C, N) f32 | bf16 read in place, obs (B, C, N)."""

    @staticmethod
    def forward(ctx, forecasts, obs, q, wgt, eps):
        B, E, Cc, N = forecasts.shape
        f = prep(forecasts)
        o = obs.float().contiguous()
        q = q.float().contiguous()
        w = wgt.float().contiguous() if wgt is not None else None
        ch = lib().mk_ens_nll_chunks(N)
        partial = torch.empty((B * Cc, ch), dtype=torch.float32, device=f.device)
        check(lib().mk_ens_nll(ptr(f), dtype_code(f), ptr(o), ptr(q), ptr(w), None, ptr(partial), None, B, E, Cc, N, float(eps), 0,
                               stream()), "mk_ens_nll")
        ctx.save_for_backward(f, o, q, w if w is not None else torch.empty(0, device=f.device))
        ctx.meta = (float(eps), w is not None, forecasts.dtype)
        return partial.sum(dim=1).reshape(B, Cc)

    @staticmethod
    def backward(ctx, g):
        f, o, q, w = ctx.saved_tensors
        eps, has_w, dt = ctx.meta
        B, E, Cc, N = f.shape
        gf = torch.empty_like(f)
        go = g.float().contiguous()
        check(lib().mk_ens_nll(ptr(f), dtype_code(f), ptr(o), ptr(q), ptr(w) if has_w else None, ptr(go), None, ptr(gf), B, E, Cc, N,
                               eps, 1, stream()), "mk_ens_nll")
        return gf.to(dt), None, None, None, None


class EnsembleNLLLoss(_EnsembleLoss):
    """``EnsembleNLLLoss`` of ``makani/utils/losses/likelihood_loss.py:30-134`` ("ensemble_nll"): the negative log likelihood of
    the observation under a Gaussian with the ensemble's mean and (``correction=0``) variance, the variance clamped at
    ``eps^2``, under the quadrature.  ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W), spatial_weights=None)
    -> (B, C)``.  Score and quadrature are one HIP kernel (``csrc/ensnll.hip``), the gradient with respect to the forecasts
    one more; 1 <= E <= 32 (more: NotImplementedError).  ``ensemble_distributed`` / ``spatial_distributed`` as ``CRPSLoss``."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, spatial_distributed: Optional[bool] = False,
                 ensemble_distributed: Optional[bool] = False, eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed)
        self.eps = eps

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        B, E, Cc, H, W = forecasts.shape               # (a forecast without an ensemble axis fails here, as in the reference)
        check_weight_dims(spatial_weights, observations, found=False)
        if not self.ensemble_distributed:           # (the members of the whole group are counted after the exchange)
            ensemble_size_check(E, "likelihood")
        need_gpu(forecasts)
        # members <-> a share of the points (:108-118), the shares summed (:127-128)
        f, o, q, w, groups = self._points(forecasts, observations, spatial_weights)
        ensemble_size_check(f.shape[1], "likelihood")
        return self._sum_shares(EnsNllFn.apply(f, o, q, w, self.eps), groups)


def _mmd_finish(sigma, alpha):
    """stage 2 of ``GaussianMMDLoss`` (``mk_mmd_finish``) between stages 1 and 3 of the energy-score pipeline: p = beta, one
    segment, a NaN observation or member masks the point"""
    def finish(sums, loss, table, B, E, Cc, nseg, reduce, p):
        check(lib().mk_mmd_finish(ptr(sums), ptr(loss), ptr(table), B, E, Cc, int(reduce), float(sigma), float(alpha), stream()),
              "mk_mmd_finish")
    return finish


class GaussianMMDLoss(_EnergyScoreMixin, _EnsembleLoss):
    """``GaussianMMDLoss`` of ``makani/utils/losses/mmd_loss.py:30-219`` ("gaussian_mmd", arXiv:1505.03906): with the distances
    s(a, b) = sum_n q w |a_n - b_n|^beta (per channel, or summed over the channels with ``channel_reduction``) and the kernel
    k = exp(-s^2 / 2 sigma):  mean_e k(o, f_e) - (E - 1 + alpha) / (2 E^2 (E - 1)) sum_{i != j} k(f_i, f_j).
    ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W), spatial_weights=None) -> (B, C) | (B, 1)``.  A point where
    the observation or any member is NaN is dropped.  Stages 1 and 3 of ``csrc/escore.hip`` with ``mk_mmd_finish`` between
    them: the members are read in place and no pair tensor exists.  1 <= E <= 32 (more: NotImplementedError).

    Deviations, stated: ``beta < 1`` raises NotImplementedError, as ``LpEnergyScoreLoss`` does for ``p < 1``.
    ``channel_reduction=True`` sums the distances over the CHANNELS and returns (B, 1), as the reference's comment, its
    ``n_channels`` and the energy scores say; the reference's ``sum(dim=-2)`` (:192-194) falls on the batch axis of its
    (E, B, C) distances and returns (1, C)."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, spatial_distributed: Optional[bool] = False,
                 ensemble_distributed: Optional[bool] = False, ensemble_weights: Optional[torch.Tensor] = None,
                 sigma: Optional[float] = 1.0, alpha: Optional[float] = 1.0, beta: Optional[float] = 2.0,
                 channel_reduction: Optional[bool] = False, **kwargs):
        if float(beta) < 1.0:
            raise NotImplementedError(f"beta = {beta}: the Gaussian MMD is built for beta >= 1 (the gradient of |d|^beta is unbounded "
                                      "at coincident members for beta < 1)")
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed)
        self.alpha, self.beta, self.channel_reduction, self.sigma = alpha, beta, channel_reduction, sigma
        self.register_buffer("ensemble_weights", ensemble_weights, persistent=False)

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: str = None) -> torch.Tensor:
        return torch.ones(1)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        self._check(forecasts, observations, spatial_weights)
        if self.ensemble_weights is not None:
            raise NotImplementedError("currently only constant ensemble weights are supported")
        if not self.ensemble_distributed:           # (the members of the whole group are counted after the exchange)
            ensemble_size_check(forecasts.shape[1], "MMD")
        need_gpu(forecasts)
        # members <-> a share of the points (:131-145), the sums added over the group (:180-182)
        f, o, q, w, groups = self._points(forecasts, observations, spatial_weights)
        ensemble_size_check(f.shape[1], "MMD")
        return EnergyScoreFn.apply(f, o, q, w, 1, 1, self.channel_reduction, self.beta, _mmd_finish(self.sigma, self.alpha), groups)


# --------------------------------------------------------------------------- #
# spectral coherence losses on the per-degree ensemble Gram matrix (energy_score.py:655-856, regularization.py:84-417)
# --------------------------------------------------------------------------- #
EGRAM_DIAG, EGRAM_OBS, EGRAM_FULL = (_lib.CONSTS["MK_EGRAM_" + k] for k in ("DIAG", "OBS", "FULL"))
EGRAM_TRI_NONE = 1 << 30          # `tri_off` of a caller that cannot name the triangle's offset: no order is skipped


def egram_slots(E, what):
    """K, the length of a row of ``mk_egram_sums`` for ``E`` members"""
    n = E + 1
    return {EGRAM_DIAG: n, EGRAM_OBS: n + E, EGRAM_FULL: n + E + E * (E - 1) // 2}[what]


def egram_slot(i, j, E):
    """slot of G[i][j] = G[j][i] in a row; fields 0 .. E - 1 are the members, field E is the observation: the diagonal, then the
    member-observation column, then the member pairs i < j in lexicographic order"""
    i, j = min(i, j), max(i, j)
    if not 0 <= i <= j <= E:
        raise IndexError(f"G[{i}][{j}] of an ensemble of {E}")
    if i == j:
        return i
    if j == E:
        return E + 1 + i
    return 2 * E + 1 + i * (2 * E - i - 1) // 2 + (j - i - 1)


def parseval_triangle_weights(lmax, mmax):
    """(lmax, mmax): 1 for m = 0, 2 for m > 0, 0 for m > l — the ``lm_weights`` / ``m_weights`` of the three reference classes"""
    w = torch.ones((lmax, mmax), dtype=torch.float32)
    w[:, 1:] *= 2.0
    ls, ms = torch.arange(lmax).reshape(-1, 1), torch.arange(mmax).reshape(1, -1)
    return torch.where(ms > ls, 0.0, w)


def egram_weights(lmax, mmax, l_off=0, m_off=0, l_loc=None, m_loc=None):
    """(q, tri_off) of ``mk_egram_sums`` for the shard [l_off, l_off + l_loc) x [m_off, m_off + m_loc) of the (lmax, mmax)
    coefficient plane: q carries every constant (1 / 4 pi — the reference's ``/ sqrt(4 pi)`` on the coefficients —, the factor
    2 of m > 0, the zeros of m > l); local order m of local degree l is structurally zero for m > l + tri_off"""
    l_loc = lmax - l_off if l_loc is None else l_loc
    m_loc = mmax - m_off if m_loc is None else m_loc
    q = parseval_triangle_weights(lmax, mmax)[l_off:l_off + l_loc, m_off:m_off + m_loc] / (4.0 * math.pi)
    return q.contiguous(), l_off - m_off


class EnsembleGramFn(torch.autograd.Function):
    """``csrc/egram.hip``: f (B, E, C, L, M) complex64 members, o (B, C, L, M) complex64 observation, q (L, M) -> G (B, C, L, K)
    f32, the Parseval-weighted Hermitian Gram matrix of the E + 1 fields per degree in the slot order of ``egram_slot``,
    truncated by ``what`` (``EGRAM_DIAG`` | ``EGRAM_OBS`` | ``EGRAM_FULL``).  The sums are added over ``sum_groups`` inside
    (the backward of a SUM all-reduce is the identity).  Gradient with respect to the members only."""

    @staticmethod
    def forward(ctx, f, o, q, what, tri_off, sum_groups):
        B, E, Cc, L, M = f.shape
        ensemble_size_check(E, "coherence")
        fr = torch.view_as_real(f.to(torch.complex64).contiguous())
        orr = torch.view_as_real(o.to(torch.complex64).contiguous())
        q = q.float().contiguous()
        if tuple(orr.shape) != (B, Cc, L, M, 2) or tuple(q.shape) != (L, M):
            raise ValueError(f"members {tuple(f.shape)}, observation {tuple(o.shape)} and weights {tuple(q.shape)} do not fit")
        G = torch.empty((B, Cc, L, egram_slots(E, what)), dtype=torch.float32, device=fr.device)
        check(lib().mk_egram_sums(ptr(fr), ptr(orr), ptr(q), ptr(G), B, E, Cc, L, M, what, int(tri_off), stream()), "mk_egram_sums")
        from . import ops
        for group in sum_groups:
            ops._all_reduce_sum(G, group)
        ctx.save_for_backward(fr, orr, q)
        ctx.meta = (what, int(tri_off))
        return G

    @staticmethod
    def backward(ctx, g):
        fr, orr, q = ctx.saved_tensors
        what, tri_off = ctx.meta
        B, E, Cc, L, M = fr.shape[:5]
        dG = g.float().contiguous()
        gf = torch.empty_like(fr)
        check(lib().mk_egram_grad(ptr(fr), ptr(orr), ptr(q), ptr(dG), ptr(gf), B, E, Cc, L, M, what, tri_off, stream()), "mk_egram_grad")
        return torch.view_as_complex(gf), None, None, None, None, None


class _EnsembleGramLoss(SpectralLpLoss):
    """what the three coherence losses share: the HIP ``RealSHT`` of members and observation (fp32, autocast off, raw
    coefficients: the 1 / 4 pi lives in the weights), ``EnsembleGramFn`` on them, and the sums over the process groups — the
    ensemble group (members <-> a share of the orders) and "w" inside the function, "h" on the loss"""

    def __init__(self, img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed, ensemble_distributed, eps):
        SpectralLpLoss.__init__(self, img_shape, crop_shape, crop_offset, channel_names, grid_type,
                                spatial_distributed=spatial_distributed, lmax=lmax, eps=eps)
        self.ensemble_distributed = ensemble_active(ensemble_distributed)
        Ll, Ml = self.lm_weights.shape
        q, self._tri_off = egram_weights(self.sht.lmax, self.sht.mmax, self._l_off, self._m_off, Ll, Ml)
        self.register_buffer("gram_weights", q, persistent=False)

    type = _EnsembleLoss.type

    @property
    def type(self):
        return "probabilistic"                                                  # LossType.Probabilistic

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)

    def _local_triangle_weights(self):
        Ll, Ml = self.gram_weights.shape
        w = parseval_triangle_weights(self.sht.lmax, self.sht.mmax)
        return w[self._l_off:self._l_off + Ll, self._m_off:self._m_off + Ml].contiguous()

    def _gram(self, forecasts, observations, what, gather_members=True):
        """forecasts (B, E, C, H, W), observations (B, C, H, W) -> G (B, C, L, K) summed over the orders of all ranks, and
        the number of members in it"""
        from . import comm as _comm
        if not (self.ensemble_distributed and gather_members):          # (else the members of the group are counted below)
            ensemble_size_check(forecasts.shape[1], "coherence")
        need_gpu(forecasts)
        with torch.autocast(device_type=forecasts.device.type, enabled=False):
            f = self.sht(forecasts.float())
            o = self.sht(observations.float())
        q, tri_off, groups = self.gram_weights, self._tri_off, []
        if self.ensemble_distributed and gather_members:
            f, o, q, group = _ensemble_split_lm(f, o, q)
            groups.append(group)
            tri_off = EGRAM_TRI_NONE                # (this rank's share of the orders: q holds the zeros, nothing is skipped)
        if self.spatial_distributed and _comm.get_size("w") > 1:
            groups.append(_comm.get_group("w"))
        E = f.shape[1]
        ensemble_size_check(E, "coherence")
        return EnsembleGramFn.apply(f, o, q, what, tri_off, groups), E

    def _sum_degrees(self, loss):
        """(B, C, L) -> (B, C): the local degrees, then the "h" group"""
        from . import comm as _comm
        loss = loss.sum(dim=-1)
        if self.spatial_distributed and _comm.get_size("h") > 1:
            loss = ReduceFromGroupFn.apply(loss, _comm.get_group("h"))
        return loss


def _pair_decoherence(psd_f, pairs, E, eps):
    """sum_{i != j} (1 - coh_ij) / (E (E - 1)) from the pair slots (each unordered pair counts twice); exactly 0 for E = 1"""
    if E < 2:
        return torch.zeros_like(psd_f[..., 0])
    iu = torch.triu_indices(E, E, 1, device=psd_f.device)          # (lexicographic: the slot order)
    coh = pairs / torch.sqrt(psd_f[..., iu[0]] * psd_f[..., iu[1]] + eps)
    return 2.0 * (1.0 - coh).sum(dim=-1) / float(E * (E - 1))


class SpectralCoherenceLoss(_EnsembleGramLoss):
    """``SpectralCoherenceLoss`` of ``makani/utils/losses/energy_score.py:655-856``: per degree l the error of the members'
    power spectral density against the observation's plus ``2 PSD_o (mean_e (1 - coh(f_e, o)) - 1/2 mean_{i != j} (1 -
    coh(f_i, f_j)))`` (``relative``: the PSD error divided by ``PSD_o + eps`` and no ``PSD_o`` factor), summed over l.
    ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W)) -> (B, C) | (B, 1)``.  HIP SHT (fp32, autocast off), then
    ONE kernel for the whole per-degree Gram matrix of members and observation (``csrc/egram.hip``, ``EGRAM_FULL``) and one for
    the gradient: no (E, E, B, C, L, M) product exists, the finish works on the (B, C, L, K) sums in fp32 torch.  ``alpha`` and
    ``ensemble_weights`` are accepted and unused, as in the reference; E = 1 gives a spread of exactly 0.
    ``spatial_distributed``: the sums are added over "w" before the finish, the loss over "h" after it; ``ensemble_distributed``:
    the members are gathered on this rank's share of the orders and the sums added over the ensemble group.

    Deviations, stated: CPU tensors raise (the HIP path has no CPU fallback); more than 32 members raise NotImplementedError."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmax: Optional[int] = None, relative: Optional[bool] = False,
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False,
                 ensemble_weights: Optional[torch.Tensor] = None, channel_reduction: Optional[bool] = True,
                 alpha: Optional[float] = 1.0, eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed,
                         ensemble_distributed, eps)
        self.relative, self.channel_reduction = relative, channel_reduction
        self.register_buffer("ensemble_weights", ensemble_weights, persistent=False)
        self.register_buffer("lm_weights", self._local_triangle_weights(), persistent=False)

    @property
    def n_channels(self):
        return 1 if self.channel_reduction else len(self.channel_names)

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: str = None) -> torch.Tensor:
        if self.channel_reduction:
            return torch.ones(1)
        return channel_weighting(self.channel_names, channel_weight_type, time_diff_scale)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, ensemble_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        check_forecast_dims(forecasts)
        G, E = self._gram(forecasts, observations, EGRAM_FULL)
        n = E + 1
        psd_f, psd_o, cross, pairs = G[..., :E], G[..., E:n], G[..., n:n + E], G[..., n + E:]
        coh_obs = cross / torch.sqrt(psd_f * psd_o + self.eps)
        psd_skill = (psd_f - psd_o).square()
        if self.relative:
            psd_skill = psd_skill / (psd_o + self.eps)
        psd_skill = psd_skill.sum(dim=-1) / float(E)
        coh_skill = (1.0 - coh_obs).sum(dim=-1) / float(E)
        coh_spread = _pair_decoherence(psd_f, pairs, E, self.eps)
        loss = 2.0 * (coh_skill - 0.5 * coh_spread)
        loss = psd_skill + (loss if self.relative else psd_o.squeeze(-1) * loss)
        loss = self._sum_degrees(loss)
        return loss.sum(dim=-1, keepdim=True) if self.channel_reduction else loss


class CoherenceRegularization(_EnsembleGramLoss):
    """``CoherenceRegularization`` of ``makani/utils/losses/regularization.py:215-417``: the mean over the band ``[lmin, lmax)``
    of ``1 - mean_e coh_l(f_e, o)`` with the signed per-degree coherence ``CrossPSD / sqrt(PSD_f PSD_o + eps)``, plus
    ``ensemble_coherence_weight * mean_{i != j} (1 - coh_l(f_i, f_j))`` when that weight is non-zero and E > 1.
    ``forward(forecasts (B, E, C, H, W), observations (B, C, H, W)) -> (B, C)``.  HIP SHT, then ``csrc/egram.hip``: ``EGRAM_FULL``
    only when the inter-member term is active, else ``EGRAM_OBS`` (PSDs and member-observation cross spectra: every member
    coefficient is read once); the finish works on the (B, C, L, K) sums in fp32 torch.  Parallel forms as
    ``SpectralCoherenceLoss``; ``band_size`` is the global width of the band.

    Deviations, stated: CPU tensors raise (the HIP path has no CPU fallback); more than 32 members raise NotImplementedError."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmin: Optional[int] = None, lmax: Optional[int] = None,
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False,
                 ensemble_weights: Optional[torch.Tensor] = None, ensemble_coherence_weight: Optional[float] = 0.0,
                 eps: Optional[float] = 1.0e-6, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed,
                         ensemble_distributed, eps)
        self.ensemble_coherence_weight = ensemble_coherence_weight
        self.register_buffer("ensemble_weights", ensemble_weights, persistent=False)
        self.lmin = lmin if lmin is not None else 0
        if self.lmin >= self.sht.lmax:
            raise ValueError(f"Error, lmin ({self.lmin}) must be smaller than the SHT truncation lmax ({self.sht.lmax}), otherwise "
                             "the band is empty.")
        l_band = torch.zeros(self.sht.lmax)
        l_band[self.lmin:self.sht.lmax] = 1.0
        band_size = l_band.sum().clamp(min=1.0)                                     # the global width (:307-310)
        Ll = self.gram_weights.shape[0]
        self.register_buffer("m_weights", self._local_triangle_weights(), persistent=False)
        self.register_buffer("l_band", l_band[self._l_off:self._l_off + Ll].contiguous(), persistent=False)
        self.register_buffer("band_size", band_size, persistent=False)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, spatial_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        if forecasts.dim() != 5:
            raise ValueError(f"Error, forecasts expected 5 dims, got {forecasts.dim()}.")
        from .comm import get_size
        E_all = forecasts.shape[1] * (get_size("ensemble") if self.ensemble_distributed else 1)
        inter = (self.ensemble_coherence_weight != 0.0) and (E_all > 1)
        G, E = self._gram(forecasts, observations, EGRAM_FULL if inter else EGRAM_OBS)
        n = E + 1
        psd_f, psd_o, cross = G[..., :E], G[..., E:n], G[..., n:n + E]
        coh_obs = cross / torch.sqrt(psd_f * psd_o + self.eps)
        loss = (1.0 - coh_obs).sum(dim=-1) / float(E)
        if inter:
            loss = loss + self.ensemble_coherence_weight * _pair_decoherence(psd_f, G[..., n + E:], E, self.eps)
        return self._sum_degrees(self.l_band * loss) / self.band_size


class SpectralRegularization(_EnsembleGramLoss):
    """``SpectralRegularization`` of ``makani/utils/losses/regularization.py:84-212``: ``sum_l |PSD_l(f_e) - PSD_l(o)|``
    (``logarithmic``: of the logarithms), averaged over the members and divided by the global ``sht.lmax``.
    ``forward(forecasts (B, E, C, H, W) | (B, C, H, W), observations (B, C, H, W)) -> (B, C)``; 4-dimensional forecasts count
    as one member.  HIP SHT, then ``csrc/egram.hip`` with ``EGRAM_DIAG`` (the diagonal only: every coefficient is read once for
    every E); the finish works on the (B, C, L, E + 1) sums in fp32 torch.  ``spatial_distributed`` as ``SpectralCoherenceLoss``;
    ``ensemble_distributed``: the members stay local, the member mean is summed over the ensemble group and divided by its size.

    Deviations, stated: CPU tensors raise (the HIP path has no CPU fallback); more than 32 local members raise
    NotImplementedError."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, lmax: Optional[int] = None, spatial_distributed: Optional[bool] = False,
                 ensemble_distributed: Optional[bool] = False, eps: Optional[float] = 1.0e-10, logarithmic: Optional[bool] = False,
                 **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, lmax, spatial_distributed,
                         ensemble_distributed, eps)
        self.logarithmic = logarithmic
        self.register_buffer("lm_weights", self._local_triangle_weights(), persistent=False)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, ensemble_weights: Optional[torch.Tensor] = None,
                **kwargs) -> torch.Tensor:
        if forecasts.dim() == 4:
            forecasts, members = forecasts.unsqueeze(1), False
        elif forecasts.dim() == 5:
            members = True
        else:
            raise ValueError(f"Error, forecasts tensor expected to have 4 or 5 dimensions but found {forecasts.dim()}.")
        G, E = self._gram(forecasts, observations, EGRAM_DIAG, gather_members=False)
        psd_f, psd_o = G[..., :E], G[..., E:]
        if self.logarithmic:
            psd_f, psd_o = torch.log(psd_f), torch.log(psd_o)
        diff = (psd_f - psd_o).abs().sum(dim=-1) / float(E)
        if members and self.ensemble_distributed:
            from . import comm as _comm
            diff = ReduceFromGroupFn.apply(diff, _comm.get_group("ensemble")) / float(_comm.get_size("ensemble"))
        return self._sum_degrees(diff) / float(self.sht.lmax)


# --------------------------------------------------------------------------- #
# hydrostatic-balance loss (makani/utils/losses/hydrostatic_loss.py) and drift regularization (regularization.py:31-81)
# --------------------------------------------------------------------------- #
class HydrostaticBalanceLoss(_Tabled):
    """``HydrostaticBalanceLoss`` of ``makani/utils/losses/hydrostatic_loss.py`` ("hydrostatic"): per interval of neighbouring
    pressure levels the quadrature of the squared residual ``(Z_{k+1} - Z_k) / R_d + 1/2 ln(p_{k+1} / p_k) (T_k + T_{k+1})`` of the
    de-normalised prediction (virtual temperature with ``use_moist_air_formula``), ``forward(prd (B, C, H, W), tar, wgt=None) ->
    (B, K - 1)`` in the dtype of ``prd``.  Constructor arguments, the non-persistent buffers ``bias``, ``scale``, ``p`` and ``cmat``
    (built by the reference's own fp32 steps, logarithms included) and both errors are the reference's.  The forward is ONE launch
    over the prediction, f32 or bf16 in place (``csrc/hydro.hip``: de-normalisation, residuals, weights and plane sums; a second,
    tiny launch adds the chunk sums in order), the backward one launch that writes the gradient of every channel.  Stated
    deviations: at most ``MAX_LEVELS`` = 16 levels (the column lives in registers; the reference has no limit); a prediction with
    ``(n_future + 1) C`` channels, on which the reference raises, is scored step by step -> ``(B, S (K - 1))``, step-major;
    ``compute_channel_weighting`` accepts the ``time_diff_scale`` keyword that ``LossHandler`` passes (the reference's method lacks
    it and dies with a ``TypeError`` there) and raises ``NotImplementedError`` for a value other than ``None``."""

    _table_sources = ("bias", "scale", "cmat")

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], grid_type: str, bias: torch.Tensor, scale: torch.Tensor, p_min: Optional[int] = 0,
                 p_max: Optional[int] = 1000, use_moist_air_formula: Optional[bool] = False,
                 spatial_distributed: Optional[bool] = False, **kwargs):
        super().__init__()
        self.img_shape, self.crop_shape, self.crop_offset = img_shape, crop_shape, crop_offset
        self.channel_names = channel_names
        self.quadrature = GridQuadrature(grid_to_quadrature_rule(grid_type), img_shape=img_shape, crop_shape=crop_shape,
                                         crop_offset=crop_offset, normalize=True, distributed=spatial_distributed)
        self.spatial_distributed = self.quadrature.distributed
        self.use_moist_air_formula = use_moist_air_formula
        self.z_idx, self.t_idx, self.pressures = get_matching_channels_pl(channel_names, "z", "t", p_min, p_max)
        if self.use_moist_air_formula:
            self.q_idx, _, p_tmp = get_matching_channels_pl(channel_names, "q", "t", p_min, p_max)
        if len(self.pressures) < 2:
            raise ValueError("Warning, we could not find at least two pressure levels which are common among z and t and inside "
                             "the specified limits")
        if self.use_moist_air_formula:
            for p1, p2 in zip(self.pressures, p_tmp):
                if p1 != p2:
                    raise ValueError("Error, make sure that you have the same pressure levels for t,z and q channels")
            if len(self.q_idx) != len(self.pressures):          # (a q column shorter than z / t: the reference fails in forward)
                raise ValueError("Error, make sure that you have the same pressure levels for t,z and q channels")
        K = len(self.pressures)
        if K > MAX_HYDRO_LEVELS:
            raise ValueError(f"Error, {K} pressure levels: the HIP path keeps a column of at most {MAX_HYDRO_LEVELS} levels in registers.")
        self.register_buffer("bias", bias, persistent=False)
        self.register_buffer("scale", scale, persistent=False)
        self.prefact = 1.0 / R_DRY_AIR
        if self.use_moist_air_formula:
            self.q_prefact = Q_CORRECTION_MOIST_AIR
        ptens = torch.as_tensor(self.pressures, dtype=torch.float32).reshape(1, -1, 1, 1)
        self.register_buffer("p", ptens, persistent=False)
        # one equation per interval; every factor by the reference's fp32 steps (a 0-dim quotient, its logarithm, times 0.5)
        cmat = torch.zeros((K - 1, len(channel_names)), dtype=torch.float32)
        for k in range(K - 1):
            half_log = 0.5 * torch.log(ptens[0, k + 1, 0, 0] / ptens[0, k, 0, 0])
            cmat[k, self.z_idx[k]] = -self.prefact
            cmat[k, self.z_idx[k + 1]] = self.prefact
            cmat[k, self.t_idx[k]] = half_log
            cmat[k, self.t_idx[k + 1]] = half_log
        self.register_buffer("cmat", cmat, persistent=False)

    @property
    def type(self):
        return "deterministic"                                                  # LossType.Deterministic

    @property
    def n_channels(self):
        return self.cmat.shape[0]

    def compute_channel_weighting(self, channel_weight_type: str, time_diff_scale: torch.Tensor = None) -> torch.Tensor:
        channel_weights = torch.ones(self.n_channels, dtype=torch.float32)
        if not channel_weight_type == "constant":
            raise NotImplementedError(f"Error, channel_weight_type {channel_weight_type} not supported for hydrostatic loss")
        if time_diff_scale is not None:
            raise NotImplementedError("Error, a time-difference scale is per channel; the hydrostatic loss has one entry per level interval")
        return channel_weights / torch.sum(channel_weights)

    def _build_tables(self, device):
        from . import ops
        K, C = len(self.pressures), len(self.channel_names)
        cm = self.cmat.detach().cpu()
        half_log = torch.stack([cm[k, self.t_idx[k]] for k in range(K - 1)])
        return ops.hydro_table(self.z_idx, self.t_idx, self.q_idx if self.use_moist_air_formula else [], C, self.bias.expand(1, C, 1, 1),
                               self.scale.expand(1, C, 1, 1), half_log, float(cm[0, self.z_idx[1]]),
                               Q_CORRECTION_MOIST_AIR if self.use_moist_air_formula else 0.0, device)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, prd: torch.Tensor, tar: torch.Tensor = None, wgt: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        from . import ops
        need_gpu(prd)
        C = len(self.channel_names)
        if prd.dim() != 4 or prd.shape[1] % C:
            raise ValueError(f"Error, the hydrostatic loss expects (B, S * {C}, H, W) predictions, got {tuple(prd.shape)}")
        q = self.quadrature.quad_weight.reshape(-1)
        if q.numel() != prd.shape[-2] * prd.shape[-1]:
            raise ValueError(f"Error, the prediction's plane {tuple(prd.shape[-2:])} is not the quadrature's {tuple(self.quadrature.quad_weight.shape[-2:])}")
        sums = ops.HydroSumsFn.apply(prd, wgt, q, self._tables(prd.device), prd.shape[1] // C)
        return self.quadrature._reduce(sums).to(prd.dtype)


class DriftRegularization(_EnsembleLoss):
    """``DriftRegularization`` of ``makani/utils/losses/regularization.py:31-81`` ("drift_regularization"): ``|quadrature(prd) -
    quadrature(tar)|^p`` per channel, the mean over the members of a 5-D prediction (summed over the "ensemble" group and divided
    by its size with ``ensemble_distributed``) -> (B, C).  The two quadratures are the plane-sum kernel of ``GridQuadrature``."""

    def __init__(self, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 channel_names: List[str], p: Optional[float] = 1.0, grid_type: Optional[str] = "equiangular",
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False, **kwargs):
        super().__init__(img_shape, crop_shape, crop_offset, channel_names, grid_type, spatial_distributed, ensemble_distributed)
        self.p = p

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None, **kwargs):
        need_gpu(prd)
        if prd.dim() > tar.dim():
            tar = tar.unsqueeze(1)
        loss = torch.abs(self.quadrature(prd) - self.quadrature(tar)).pow(self.p)
        if prd.dim() == 5:
            loss = torch.mean(loss, dim=1)
            if self.ensemble_distributed:
                from . import comm as _comm
                loss = ReduceFromGroupFn.apply(loss, _comm.get_group("ensemble")) / float(_comm.get_size("ensemble"))
        return loss


# --------------------------------------------------------------------------- #
# LossHandler (makani/utils/loss.py:57-494)
# --------------------------------------------------------------------------- #
_LOSS_REGISTRY = {
    "l1": partial(GeometricLpLoss, p=1),
    "l2": partial(GeometricLpLoss, p=2),
    "spectral l1": partial(SpectralLpLoss, p=1),
    "spectral l2": partial(SpectralLpLoss, p=2),
    "h1": SpectralH1Loss,
    "amse": SpectralAMSELoss,
    "hydrostatic": HydrostaticBalanceLoss,
    "ensemble_crps": CRPSLoss,
    "ensemble_spectral_crps": SpectralCRPSLoss,
    "ensemble_vort_div_crps": VortDivCRPSLoss,
    "ensemble_gradient_crps": GradientCRPSLoss,
    "ensemble_nll": EnsembleNLLLoss,
    "gaussian_mmd": GaussianMMDLoss,
    "lp_energy_score": LpEnergyScoreLoss,
    "l2_energy_score": partial(LpEnergyScoreLoss, p=2.0),
    "sobolev_energy_score": SobolevEnergyScoreLoss,
    "spectral_l2_energy_score": SpectralL2EnergyScoreLoss,
    "drift_regularization": DriftRegularization,
    "spectral_regularization": SpectralRegularization,
}


def _params_get(params, key, default=None):
    return params.get(key, default) if hasattr(params, "get") else getattr(params, key, default)


class LossHandler(nn.Module):
    """``LossHandler`` of ``makani/utils/loss.py:57-494``: builds the losses of ``params.losses`` (or ``params.loss``) from the
    registry, owns their channel weights, relative weights, multistep weights and running statistics, and in ``forward(prd, tar,
    wgt=None, inp=None, training_progress=None)`` hands every loss the tensors it scores — the ensemble mean for the deterministic
    ones, tendencies against the last input step where a loss asks for them — and returns the weighted scalar.  Buffers, their
    persistence and shapes are the reference's (a reference ``state_dict`` loads strictly), as are the per-loss keys
    (``parameters``, ``channel_weights``, ``relative_weight``, ``temp_diff_normalization``, ``tendency``), the six multistep weight
    types and every error.  The four tensors the reference forms in separate torch passes (``mean_E(prd)``, ``prd - inp``,
    ``mean - inp``, ``tar - inp``) come from ONE launch that writes only what some loss reads (``ops.LossPrepFn``).

    Under ``n_future > 0`` every loss returns step-major vectors ``[step 0: its channels | step 1: its channels | ..]`` and the
    handler concatenates them per LOSS, while the weights are the per-loss weights concatenated and then tiled per STEP
    (``loss.py:457,488``): with more than one loss the two orders differ, and a weight can meet another loss's value.  This is
    reproduced as it is (the recorded reference values pin it), not repaired.

    Stated deviations: ``bias``, ``scale`` (1, C, 1, 1) and ``time_diff_stds`` (C) are tensors of the OUTPUT channels (the reference
    reads the files named in ``params``); ``compile`` is accepted and ignored; ``random_slice_loss=True`` raises
    ``NotImplementedError`` (a C x C channel mix; this project ships no library GEMM); ``uncertainty_weighting`` /
    ``balanced_weighting`` choose "ones until 100 batches" with ``torch.where`` on the device counter (the reference reads it with
    ``.item()``); ``randomized_loss_weights`` draws from a device ``torch.Generator`` seeded with ``seed``; a tendency needs as many
    input as prediction channels at any ``n_future`` (the reference checks at ``n_future = 0`` and fails in the subtraction
    otherwise); CPU tensors raise.  Except for the randomized draw nothing is read on the host: forward and backward replay from a
    captured graph."""

    def __init__(self, params, track_running_stats: bool = False, seed: int = 0, eps: float = 1e-6, compile: bool = True, *,
                 bias: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                 time_diff_stds: Optional[torch.Tensor] = None, **kwargs):
        super().__init__()
        from . import comm as _comm
        _comm.autodetect()
        self.rank = _comm.get_rank("matmul")
        self.n_future = params.n_future
        self.n_history = params.n_history
        self.spatial_distributed = _comm.is_distributed("spatial") and (_comm.get_size("spatial") > 1)
        self.ensemble_distributed = _comm.is_distributed("ensemble") and (_comm.get_size("ensemble") > 1)
        self.img_shape = (params.img_shape_x_resampled, params.img_shape_y_resampled)
        self.crop_shape = (params.img_shape_x_resampled, params.img_shape_y_resampled)
        self.crop_offset = (params.img_crop_offset_x, params.img_crop_offset_y)
        self.uncertainty_weighting = _params_get(params, "uncertainty_weighting", False)
        self.balanced_weighting = _params_get(params, "balanced_weighting", False)
        self.randomized_loss_weights = _params_get(params, "randomized_loss_weights", False)
        self.random_slice_loss = _params_get(params, "random_slice_loss", False)
        if self.random_slice_loss:
            raise NotImplementedError("random_slice_loss mixes the channels with a C x C matrix per call; it is not built on the HIP path")
        self.track_running_stats = track_running_stats or self.uncertainty_weighting or self.balanced_weighting
        self.eps = eps
        self.seed = seed

        if hasattr(params, "losses"):
            losses = params.losses
        elif hasattr(params, "loss"):
            losses = [{"type": params.loss}]
        else:
            raise ValueError("No loss function specified.")

        n_out = len(params.channel_names)
        bias = torch.zeros((1, n_out, 1, 1), dtype=torch.float32) if bias is None else torch.as_tensor(bias).detach().to(torch.float32).cpu()
        scale = torch.ones((1, n_out, 1, 1), dtype=torch.float32) if scale is None else torch.as_tensor(scale).detach().to(torch.float32).cpu()

        self.loss_fn = nn.ModuleList([])
        self.loss_requires_input = []
        self.loss_types = []
        channel_weights = []
        for loss in losses:
            requires_input = loss.get("tendency", False)
            loss_params = loss.get("parameters", {})
            loss_handle = self._parse_loss_type(loss["type"])
            loss_fn = loss_handle(img_shape=self.img_shape, crop_shape=self.crop_shape, crop_offset=self.crop_offset,
                                  channel_names=params.channel_names, bias=bias, scale=scale, grid_type=params.model_grid_type,
                                  spatial_distributed=self.spatial_distributed, ensemble_distributed=self.ensemble_distributed,
                                  **loss_params)
            self.loss_types.append(loss_fn.type)
            self.loss_fn.append(loss_fn)
            self.loss_requires_input.append(requires_input)

            channel_weight_type = loss["channel_weights"] if "channel_weights" in loss.keys() else "constant"
            if loss.get("temp_diff_normalization", False):
                if time_diff_stds is None:
                    raise ValueError("time_diff_std_path not defined.")          # (here: the time_diff_stds tensor was not given)
                tds = torch.clamp(torch.as_tensor(time_diff_stds).detach().to(torch.float32).cpu().flatten(), min=1e-4)
                time_diff_scale = scale.flatten() / tds
            else:
                time_diff_scale = None
            if isinstance(channel_weight_type, list):
                chw = torch.tensor(channel_weight_type, dtype=torch.float32)
                if time_diff_scale is not None:
                    chw = chw * time_diff_scale
                if chw.shape[1] != loss_fn.n_channels:
                    raise ValueError(f"expected channel weights to have {loss_fn.n_channels} channels, but got {chw.shape[1]}")
            else:
                with _handler_weights():
                    chw = loss_fn.compute_channel_weighting(channel_weight_type, time_diff_scale=time_diff_scale)
                chw = torch.as_tensor(chw, dtype=torch.float32)
            chw = chw.reshape(1, -1).clone()
            if "relative_weight" in loss.keys():
                chw *= loss["relative_weight"]
            channel_weights.append(chw)

        channel_weights = torch.cat(channel_weights, dim=1)
        ncw = channel_weights.shape[1]
        self.register_buffer("channel_weights", channel_weights, persistent=False)
        stats_buffer_shape = (self.n_future + 1) * channel_weights.shape[-1]
        self.register_buffer("running_mean", torch.zeros(stats_buffer_shape), persistent=True)
        self.register_buffer("running_var", torch.ones(stats_buffer_shape), persistent=True)
        self.register_buffer("num_batches_tracked", torch.tensor([0], dtype=torch.long), persistent=True)
        multistep_params = _params_get(params, "multistep", {"weight_type": "constant"})
        multistep_weight = self._compute_multistep_weight(**multistep_params)
        # (the step weight is the slow index, the channel the fast one)
        multistep_weight = torch.repeat_interleave(multistep_weight.reshape(1, -1), ncw, dim=1)
        self.register_buffer("multistep_weight", multistep_weight, persistent=False)
        self._rng = None

    def _compute_multistep_weight(self, **kwargs) -> torch.Tensor:
        weight_type = kwargs.get("weight_type", "constant")
        n = self.n_future + 1
        if weight_type == "constant":
            w = torch.ones(n, dtype=torch.float32) / float(n)
        elif weight_type == "balanced":          # the n-th step is back-propagated n times
            w = 2.0 * torch.arange(1, n + 1, dtype=torch.float32) / float((n + 1) * n)
        elif weight_type == "linear":
            w = torch.arange(1, n + 1, dtype=torch.float32) / float(n)
        elif weight_type == "last-n-1":
            w = torch.ones(n, dtype=torch.float32) / float(self.n_future)
            w[0] = 0.0
        elif weight_type == "last":
            w = torch.zeros(n, dtype=torch.float32)
            w[-1] = 1.0
        elif weight_type == "custom":
            w = torch.as_tensor(kwargs["weights"], dtype=torch.float32)
            if w.shape[0] != n:
                raise ValueError(f"Number of multistep weights ({w.shape[0]}) must match n_future+1 ({n})")
        else:
            raise ValueError(f"Unknown multistep loss weight type: {weight_type}")
        return w

    def _parse_loss_type(self, loss_type: str):
        if loss_type not in _LOSS_REGISTRY:
            raise NotImplementedError(f"Unknown loss function: {loss_type}")
        return _LOSS_REGISTRY[loss_type]

    def _gather_batch(self, x: torch.Tensor) -> torch.Tensor:
        from . import comm as _comm
        if _comm.is_distributed("batch") and _comm.get_size("batch") > 1:
            from . import ops
            n, me = _comm.get_size("batch"), _comm.get_rank("batch")
            parts = torch.zeros((n, *x.shape), dtype=x.dtype, device=x.device)          # every rank fills its own rows, the sum gathers
            parts[me] = x
            ops._all_reduce_sum(parts, _comm.get_group("batch"))
            x = parts.reshape(n * x.shape[0], *x.shape[1:])
        return x

    def is_distributed(self):
        return False

    def _update_running_stats(self, x: torch.Tensor):
        """Chan, Golub and LeVeque's parallel update of mean and second moment with the batch's"""
        with torch.no_grad():
            num_batches = torch.ones_like(x[:, 0], dtype=torch.long)
            num_batches = self._gather_batch(num_batches).sum()
            x = self._gather_batch(x)
            var, mean = torch.var_mean(x, dim=(0), correction=0, keepdim=False)
            m2 = var * num_batches
            delta = mean - self.running_mean
            self.running_var += m2 + delta**2 * self.num_batches_tracked * num_batches / (self.num_batches_tracked + num_batches)
            self.running_mean += delta * num_batches / (self.num_batches_tracked + num_batches)
            self.num_batches_tracked += num_batches

    def get_running_stats(self, correction: int = 0):
        if not self.track_running_stats:
            raise ValueError("Module does not track running stats")
        var = self.running_var / (self.num_batches_tracked - int(correction))
        return var, self.running_mean

    def reset_running_stats(self):
        with torch.no_grad():
            self.running_mean.zero_()
            self.running_var.fill_(1)
            self.num_batches_tracked.zero_()

    def _extract_input_state(self, inp: torch.Tensor) -> torch.Tensor:
        """the last step of a flattened history (B, (n_history + 1) C, H, W) -> (B, C, H, W), a view"""
        n_channels_per_step = inp.shape[1] // (self.n_history + 1)
        return inp[..., -n_channels_per_step:, :, :]

    def _prepare(self, prd, tar, inp):
        """(prdm, prd_t, prdm_t, tar_t): the ensemble mean, the member / mean / target tendencies; what no loss reads is None"""
        from . import comm as _comm
        from . import ops
        ens = prd.dim() == 5
        tend = inp is not None and any(self.loss_requires_input)
        uses = set(zip(self.loss_types, (bool(r) and tend for r in self.loss_requires_input)))
        inp_state = None
        if tend:
            inp_state = self._extract_input_state(inp)
            if prd.shape[-3] != inp_state.shape[1]:
                raise ValueError(f"Channel mismatch: prediction has {prd.shape[-3]} channels but input has {inp_state.shape[1]} channels")
        flags = 0
        if ens and ("deterministic", False) in uses:
            flags |= ops.PREP_MEAN
        if ("deterministic", True) in uses or (not ens and ("probabilistic", True) in uses):
            flags |= ops.PREP_MEAN_T
        if ens and ("probabilistic", True) in uses:
            flags |= ops.PREP_MEMBER_T
        if tend:
            flags |= ops.PREP_TAR_T
        if flags == 0:
            return prd, None, None, None
        p5 = prd if ens else prd.unsqueeze(1)
        E = p5.shape[1]
        if ens and self.ensemble_distributed:          # the local sum over 1 / (E_loc * group size), summed over the group (loss.py:395-397)
            group, gsize = _comm.get_group("ensemble"), _comm.get_size("ensemble")
            first = (flags & ~ops.PREP_MEAN_T) | (ops.PREP_MEAN if flags & (ops.PREP_MEAN | ops.PREP_MEAN_T) else 0)
            prdm, prd_t, _, tar_t = ops.LossPrepFn.apply(p5, tar, inp_state, first, 1.0 / float(E * gsize))
            prdm_t = None
            if prdm is not None:
                prdm = ReduceFromGroupFn.apply(prdm, group)
                if flags & ops.PREP_MEAN_T:
                    prdm_t = ops.LossPrepFn.apply(prdm.unsqueeze(1), tar, inp_state, ops.PREP_MEAN_T, 1.0)[2]
            return prdm, prd_t, prdm_t, tar_t
        prdm, prd_t, prdm_t, tar_t = ops.LossPrepFn.apply(p5, tar, inp_state, flags, 1.0 / float(E))
        if not ens:
            prdm, prd_t = prd, prdm_t
        return prdm, prd_t, prdm_t, tar_t

    @device_guard
    def forward(self, prd: torch.Tensor, tar: torch.Tensor, wgt: Optional[torch.Tensor] = None, inp: Optional[torch.Tensor] = None,
                training_progress: Optional[float] = None, **kwargs):
        # prd (B, E, C, H, W) or (B, C, H, W)
        need_gpu(prd)
        prdm, prd_t, prdm_t, tar_t = self._prepare(prd, tar, inp)
        tend = tar_t is not None
        loss_vals = []
        for lfn, requires_inp, loss_type in zip(self.loss_fn, self.loss_requires_input, self.loss_types):
            if self.n_future > 0:
                lead_time_step = torch.arange(0, self.n_future + 1, dtype=torch.long, device=prd.device).repeat_interleave(lfn.n_channels)
            else:
                lead_time_step = None
            kwargs_step = {"lead_time_step": lead_time_step, "training_progress": training_progress, "n_future": self.n_future}
            if loss_type == "deterministic":
                a, b = (prdm_t, tar_t) if (requires_inp and tend) else (prdm, tar)
            else:
                a, b = (prd_t, tar_t) if (requires_inp and tend) else (prd, tar)
            loss_vals.append(lfn(a, b, wgt, **kwargs_step))
        all_losses = torch.cat(loss_vals, dim=-1)

        if self.training and self.track_running_stats:
            self._update_running_stats(all_losses.clone())

        chw = self.channel_weights
        if self.uncertainty_weighting and self.training:
            var, _ = self.get_running_stats()
            var = torch.where(self.num_batches_tracked <= 100, torch.ones_like(var), var)
            chw = chw / (torch.sqrt(2 * var) + self.eps)
        elif self.balanced_weighting and self.training:
            _, mean = self.get_running_stats()
            mean = torch.where(self.num_batches_tracked <= 100, torch.ones_like(mean), mean)
            chw = chw / (mean + self.eps)

        if self.randomized_loss_weights:
            if self._rng is None or self._rng.device != chw.device:
                self._rng = torch.Generator(device=chw.device)
                self._rng.manual_seed(self.seed)
            rmask = torch.zeros_like(chw)
            rmask.uniform_(0.0, 1.0, generator=self._rng)
            chw = chw * (rmask / rmask.sum())

        if self.training:
            if self.n_future > 0:          # the per-loss weights, concatenated, tiled per step: see the class docstring
                chw = torch.tile(chw, (1, self.n_future + 1))
            chw = chw * self.multistep_weight

        return torch.mean(torch.sum(chw * all_losses, dim=1), dim=0)
