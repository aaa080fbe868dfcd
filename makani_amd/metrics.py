"""The geometric validation metrics on the HIP path: ``GeometricL1``, ``GeometricRMSE``, ``GeometricACC``, ``GeometricSpread``,
``GeometricSSR``, ``GeometricCRPS`` and ``GeometricRankHistogram`` of ``makani/utils/metrics/functions.py:29-677`` on the base
class of ``makani/utils/metrics/base_metric.py:68-185``: same constructor arguments and defaults, same ``type``,
``compute_counts``, ``combine``, ``finalize``, same ``ValueError`` messages.

Every metric is a quadrature over the plane followed by arithmetic on ``(B, C[, k])`` numbers.  The quadratures are two HIP
kernels (``csrc/metrics.hip``): ``mk_metric_det_sums`` forms the five sums behind L1, RMSE and ACC in one read of prediction
and target (``deterministic_sums``: a caller that wants RMSE and ACC of the same pair pays one pass), ``mk_metric_ens_sums``
forms skill, spread and the rank histogram of an ensemble in one read of the members, without the ensemble-sized difference
tensor, the sort or the one-hot tensor of the reference.  What follows the sums (``sqrt``, the ACC ratio with ``eps``, SSR's
clamp, ``/ (E - 1)``, channel and batch reductions) is plain torch on the small tensor, in the reference's order, so an
ensemble of one member yields what the reference's arithmetic yields (NaN for spread and SSR).

``spatial_distributed`` adds the sums over the spatial group before the finish.  ``ensemble_distributed`` (SSR, rank histogram;
Spread whenever the "ensemble" group has more than one rank, as the reference) trades this rank's members for all members on a
share of the points (``ensemble.ensemble_split``) and adds the sums over the ensemble group: no field-sized all-reduce of the
mean.  ACC's ``bias`` is cut to the local lat/lon shard at construction (functions.py:165-169).

Deviations from the reference, stated:
  * results carry no autograd graph (the metrics run under ``no_grad`` in the validation loop);
  * a CPU tensor raises ``RuntimeError``, as the losses of this package do: there is no CPU fallback;
  * rank-histogram inputs must be finite: the rank is the number of members ``<=`` the observation, which equals
    ``sort`` + ``searchsorted(side="right")`` for finite values only (``torch.sort`` places NaN last, a comparison is false);
  * ensembles of 1..32 members per point (more: ``NotImplementedError``);
  * GeometricACC's ``bias`` is a climatology without a batch axis (``(C, H, W)``, ``(1, C, H, W)`` or broadcastable to it);
  * GeometricSSR built without ``ensemble_distributed`` in a job with a split ensemble group scores this rank's members as a
    complete ensemble (the reference divides the local member sum by the global member count there)."""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import comm as _comm
from ._lib import CONSTS, check, device_guard, dtype_code, lib, need_gpu, prep, ptr, stream
from .ensemble import check_forecast_dims, check_weight_dims, ensemble_active, ensemble_size_check, flatten_and_split
from .losses import CRPSLoss, GridQuadrature, grid_to_quadrature_rule

# MK_METRIC_* of include/makani_amd.h: bit k selects [..., k]
SUM_L1, SUM_L2, SUM_XY, SUM_XX, SUM_YY = (CONSTS["MK_METRIC_" + k] for k in ("L1", "L2", "XY", "XX", "YY"))
SUM_ALL = SUM_L1 | SUM_L2 | SUM_XY | SUM_XX | SUM_YY
SUM_ACC = SUM_XY | SUM_XX | SUM_YY
ENS_SKILL, ENS_SPREAD, ENS_HIST = (CONSTS["MK_METRIC_" + k] for k in ("SKILL", "SPREAD", "HIST"))


class LossType(object):
    """``makani/utils/losses/base_loss.py:244-246``: the values ``MetricsHandler`` compares ``metric.type`` with"""
    Deterministic = 1
    Probabilistic = 2


def _sanitize_shapes(vals, counts, dim):
    """``base_metric.py:28-48``: counts broadcast against vals along ``dim``"""
    if vals.dim() == counts.dim():
        for vdim, cdim in zip(vals.shape, counts.shape):
            if vdim != cdim and vdim != 1 and cdim != 1:
                raise ValueError("The shape of vals and counts have to match or be one")
        return vals, counts
    if counts.dim() != 1:
        raise ValueError("The shape of counts has to be exactly 1")
    cshape = [1 for _ in range(vals.dim())]
    cshape[dim] = -1
    return vals, counts.reshape(cshape)


def _welford_reduction_helper(vals, counts, batch_reduction, dim):
    """``base_metric.py:51-64``"""
    counts_res = torch.sum(counts, dim=dim)
    if batch_reduction == "mean":
        vals_res = torch.sum(vals * counts, dim=dim) / counts_res
    elif batch_reduction == "sum":
        vals_res = torch.sum(vals, dim=dim)
    else:
        vals_res, counts_res = vals, counts
    return vals_res, counts_res


def _reduce(v, channel_reduction, batch_reduction):
    if channel_reduction == "mean":
        v = torch.mean(v, dim=1)
    elif channel_reduction == "sum":
        v = torch.sum(v, dim=1)
    if batch_reduction == "mean":
        v = torch.mean(v, dim=0)
    elif batch_reduction == "sum":
        v = torch.sum(v, dim=0)
    return v


def _det_launch(x, y, q, bias, w, which):
    """x, y (B, C, N) f32 | bf16, q (N), bias (C, N) | None, w (B, C, N) | None -> (B, C, 5); unselected entries are 0"""
    B, C, N = x.shape
    ch = lib().mk_metric_chunks(N)
    out = torch.zeros((B, C, 5), dtype=torch.float32, device=x.device)
    ws = torch.empty((B * C * ch * 5,), dtype=torch.float32, device=x.device)
    check(lib().mk_metric_det_sums(ptr(x), dtype_code(x), ptr(y), dtype_code(y), ptr(bias), ptr(w), ptr(q), ptr(out), ptr(ws),
                                   B, C, N, int(which), stream()), "mk_metric_det_sums")
    return out


def _ens_launch(f, o, q, w, which):
    """f (B, E, C, N) f32 | bf16, o (B, C, N) f32, q (N), w (B, C, N) | None -> (B, C, E + 3): skill, spread, E + 1 bins"""
    B, E, C, N = f.shape
    ch = lib().mk_metric_chunks(N)
    out = torch.zeros((B, C, E + 3), dtype=torch.float32, device=f.device)
    ws = torch.empty((B * C * ch * (E + 3),), dtype=torch.float32, device=f.device)
    check(lib().mk_metric_ens_sums(ptr(f), dtype_code(f), ptr(o), ptr(w), ptr(q), ptr(out), ptr(ws), B, E, C, N, int(which),
                                   stream()), "mk_metric_ens_sums")
    return out


def _bias_plane(bias, C, H, W):
    b = bias
    while b.dim() > 3 and b.shape[0] == 1:
        b = b[0]
    if b.dim() > 3:
        raise ValueError(f"the bias of GeometricACC is a climatology without a batch axis, found shape {tuple(bias.shape)}")
    return b.float().expand(C, H, W).contiguous().reshape(C, H * W)


@torch.no_grad()
def deterministic_sums(x: torch.Tensor, y: torch.Tensor, quadrature: GridQuadrature, bias: Optional[torch.Tensor] = None,
                       weight: Optional[torch.Tensor] = None, which: int = SUM_ALL) -> torch.Tensor:
    """``(B, C, 5)`` fp32: the quadratures ``sum q w {|x - y|, (x - y)^2, x'y', x'^2, y'^2}`` with ``x' = x - bias``, ``y' = y - bias``
    of ``x``, ``y`` ``(B, C, H, W)`` (f32 or bf16, each with its own dtype) in ONE pass over both; ``which`` (``SUM_L1 | SUM_L2 |
    SUM_XY | SUM_XX | SUM_YY``) names the sums to form, the others stay 0.  ``quadrature`` supplies the weights of the (local)
    grid and, when it is distributed, the sum over the spatial group."""
    B, C, H, W = x.shape
    xs = prep(x).reshape(B, C, H * W)
    ys = prep(y, x.shape).reshape(B, C, H * W)
    w = weight.float().expand(B, C, H, W).contiguous().reshape(B, C, H * W) if weight is not None else None
    b = _bias_plane(bias, C, H, W) if (bias is not None and (which & SUM_ACC)) else None
    q = quadrature.quad_weight.reshape(-1)
    if q.numel() != H * W:
        raise ValueError(f"the quadrature holds {q.numel()} weights for planes of {H} x {W} points")
    need_gpu(x, "metrics")
    return quadrature._reduce(_det_launch(xs, ys, q, b, w, which))


class GeometricBaseMetric(nn.Module):
    """``base_metric.py:68-185``"""
    _channel_dim = 1          # the channel axis of the first forward argument: 2 behind an ensemble axis

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Optional[Tuple[int, int]] = None,
                 crop_offset: Optional[Tuple[int, int]] = (0, 0), normalize: Optional[bool] = True,
                 channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean",
                 spatial_distributed: Optional[bool] = False):
        super().__init__()
        self.img_shape, self.crop_shape, self.crop_offset = img_shape, crop_shape, crop_offset
        self.channel_reduction, self.batch_reduction = channel_reduction, batch_reduction
        self.quadrature = GridQuadrature(grid_to_quadrature_rule(grid_type), img_shape=img_shape, crop_shape=crop_shape,
                                         crop_offset=crop_offset, normalize=normalize, distributed=spatial_distributed)
        self.spatial_distributed = self.quadrature.distributed

    @property
    def type(self):
        return LossType.Deterministic

    def compute_counts(self, inp: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        return _compute_counts(self, inp, weight, self._channel_dim)

    def combine(self, vals: torch.Tensor, counts: torch.Tensor, dim: Optional[int] = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        vals, counts = _sanitize_shapes(vals, counts, dim=dim)
        return _welford_reduction_helper(vals, counts, self.batch_reduction, dim=dim)

    def finalize(self, vals: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
        return vals if self.batch_reduction == "mean" else vals / counts

    @torch.no_grad()
    def _ensemble_sums(self, forecasts, observations, weight, which, ensemble_distributed, check_weights=False):
        """(sums (B, C, E_tot + 3) over the whole sphere and the whole ensemble, E_tot)"""
        check_forecast_dims(forecasts)
        if check_weights:
            check_weight_dims(weight, observations)
        B, E, C, H, W = forecasts.shape
        if not ensemble_distributed:
            ensemble_size_check(E, "metric")
        if self.quadrature.quad_weight.numel() != H * W:
            raise ValueError(f"the quadrature holds {self.quadrature.quad_weight.numel()} weights for planes of {H} x {W} points")
        need_gpu(forecasts, "metrics")
        # (the kernel takes its operands as they are: dense fp32 observations and weights of the full shape)
        f = prep(forecasts)
        o = observations.float().expand(B, C, H, W).contiguous()
        w = weight.float().expand(B, C, H, W).contiguous() if weight is not None else None
        # members <-> a share of the points; the shares are summed below
        f, o, q, w, group = flatten_and_split(f, o, self.quadrature.quad_weight.reshape(-1), w, ensemble_distributed)
        ensemble_size_check(f.shape[1], "metric")
        sums = _ens_launch(f, o, q, w, which)
        if ensemble_distributed:
            from . import ops
            ops._all_reduce_sum(sums, group)
        return self.quadrature._reduce(sums), f.shape[1]


def _compute_counts(self, inp, weight, cdim):
    if weight is not None:
        if self.batch_reduction == "mean":
            raise ValueError("Batch reduction mode 'mean' is not supported when weights are provided. Use 'sum' instead.")
        elif self.batch_reduction == "sum":
            counts = torch.sum(self.quadrature(weight.to(dtype=inp.dtype)), dim=0)
        else:
            raise ValueError(f"Batch reduction mode '{self.batch_reduction}' is not supported")
    else:
        if self.batch_reduction == "mean":
            counts = torch.ones(size=(inp.shape[cdim],), device=inp.device, dtype=inp.dtype)
        elif self.batch_reduction == "sum":
            counts = torch.full(size=(inp.shape[cdim],), fill_value=inp.shape[0], device=inp.device, dtype=inp.dtype)
        else:          # (the reference leaves counts unbound here; MetricRollout refuses batch_reduction="none" up front)
            raise ValueError(f"Batch reduction mode '{self.batch_reduction}' is not supported")
    if self.channel_reduction == "mean":
        counts = torch.mean(counts, dim=0)
    elif self.channel_reduction == "sum":
        counts = torch.sum(counts, dim=0)
    return counts


class GeometricL1(GeometricBaseMetric):
    """``functions.py:29-71``: the quadrature of ``|x - y| * weight``"""

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Optional[Tuple[int, int]] = None,
                 crop_offset: Optional[Tuple[int, int]] = (0, 0), normalize: Optional[bool] = False,
                 channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean",
                 spatial_distributed: Optional[bool] = False, **kwargs):
        super().__init__(grid_type=grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction, spatial_distributed=spatial_distributed)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        diff = deterministic_sums(x, y, self.quadrature, weight=weight, which=SUM_L1)[..., 0]
        return _reduce(diff, self.channel_reduction, self.batch_reduction)


class GeometricRMSE(GeometricBaseMetric):
    """``functions.py:74-132``: the square root of the reduced quadrature of ``(x - y)^2 * weight``; ``combine`` averages squares"""

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Optional[Tuple[int, int]] = None,
                 crop_offset: Optional[Tuple[int, int]] = (0, 0), normalize: Optional[bool] = False,
                 channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean",
                 spatial_distributed: Optional[bool] = False, **kwargs):
        super().__init__(grid_type=grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction, spatial_distributed=spatial_distributed)

    def combine(self, vals, counts, dim=0):
        vals, counts = _sanitize_shapes(vals, counts, dim=dim)
        vals_res, counts_res = _welford_reduction_helper(torch.square(vals), counts, self.batch_reduction, dim=dim)
        return torch.sqrt(vals_res), counts_res

    def finalize(self, vals, counts):
        return vals if self.batch_reduction == "mean" else vals / torch.sqrt(counts)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        diff = deterministic_sums(x, y, self.quadrature, weight=weight, which=SUM_L2)[..., 1]
        return torch.sqrt(_reduce(diff, self.channel_reduction, self.batch_reduction))


class GeometricACC(GeometricBaseMetric):
    """``functions.py:135-218``: anomaly correlation; ``method="macro"`` forms the ratio per sample, ``"micro"`` returns
    ``[cov_xy, var_x, var_y]`` stacked along the last axis and forms it in ``finalize``"""

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Optional[Tuple[int, int]] = None,
                 crop_offset: Optional[Tuple[int, int]] = (0, 0), normalize: Optional[bool] = False,
                 channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean",
                 method: Optional[str] = "macro", bias: Optional[torch.Tensor] = None, eps: Optional[float] = 1e-8,
                 spatial_distributed: Optional[bool] = False, **kwargs):
        super().__init__(grid_type=grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction, spatial_distributed=spatial_distributed)
        self.method, self.eps = method, eps
        if bias is not None:
            from . import distributed as thd
            if _comm.get_size("w") > 1:
                bias = thd.split_tensor_along_dim(bias, dim=-1, num_chunks=_comm.get_size("w"))[_comm.get_rank("w")]
            if _comm.get_size("h") > 1:
                bias = thd.split_tensor_along_dim(bias, dim=-2, num_chunks=_comm.get_size("h"))[_comm.get_rank("h")]
            self.register_buffer("bias", bias, persistent=False)

    def compute_counts(self, inp: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        counts = super().compute_counts(inp, weight)
        return counts.unsqueeze(-1) if self.method == "micro" else counts

    def finalize(self, vals, counts):
        if self.method == "micro":
            return vals[..., 0] / torch.sqrt(vals[..., 1] * vals[..., 2])
        return super().finalize(vals, counts)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        sums = deterministic_sums(x, y, self.quadrature, bias=getattr(self, "bias", None), weight=weight, which=SUM_ACC)
        if self.method == "macro":
            acc = sums[..., 2] / (torch.sqrt(sums[..., 3] * sums[..., 4]) + self.eps)
        else:
            acc = sums[..., 2:5]
        return _reduce(acc, self.channel_reduction, self.batch_reduction)


class GeometricSpread(GeometricBaseMetric):
    """``functions.py:221-317``: ``sqrt(quadrature(sum_e (mean - f_e)^2) / (E - 1))``"""
    _channel_dim = 2

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Optional[Tuple[int, int]] = None,
                 crop_offset: Optional[Tuple[int, int]] = (0, 0), normalize: Optional[bool] = False,
                 channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean",
                 spatial_distributed: Optional[bool] = False, **kwargs):
        super().__init__(grid_type=grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction, spatial_distributed=spatial_distributed)
        _comm.autodetect()
        self.ensemble_distributed = _comm.is_distributed("ensemble") and _comm.get_size("ensemble") > 1      # (:288, :302: no flag)

    @property
    def type(self):
        return LossType.Probabilistic

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        sums, ens_size = self._ensemble_sums(forecasts, observations, weight, ENS_SPREAD, self.ensemble_distributed)
        spread = torch.sqrt(sums[..., 1] / float(ens_size - 1))
        return _reduce(spread, self.channel_reduction, self.batch_reduction)


class GeometricSSR(GeometricBaseMetric):
    """``functions.py:320-430``: spread-skill ratio ``sqrt(spread / clamp(skill - spread / E, min=eps))``"""
    _channel_dim = 2

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Optional[Tuple[int, int]] = None,
                 crop_offset: Optional[Tuple[int, int]] = (0, 0), normalize: Optional[bool] = False,
                 channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean", eps: Optional[float] = 1e-6,
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False, **kwargs):
        super().__init__(grid_type=grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction, spatial_distributed=spatial_distributed)
        self.ensemble_distributed = ensemble_active(ensemble_distributed)
        self.eps = eps

    @property
    def type(self):
        return LossType.Probabilistic

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        sums, ens_size = self._ensemble_sums(forecasts, observations, weight, ENS_SKILL | ENS_SPREAD, self.ensemble_distributed)
        skill, spread = sums[..., 0], sums[..., 1] / float(ens_size - 1)
        ssr = torch.sqrt(spread / torch.clamp(skill - spread / float(ens_size), min=self.eps))
        return _reduce(ssr, self.channel_reduction, self.batch_reduction)


class GeometricCRPS(nn.Module):
    """``functions.py:433-529``: ``CRPSLoss`` of this package with the metric's reductions, counts, ``combine`` and ``finalize``"""

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 crps_type: Optional[str] = "skillspread", channel_reduction: Optional[str] = "mean",
                 batch_reduction: Optional[str] = "mean", ensemble_weights: Optional[torch.Tensor] = None,
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False, **kwargs):
        super().__init__()
        self.metric_func = CRPSLoss(img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, channel_names=[],
                                    grid_type=grid_type, crps_type=crps_type, spatial_distributed=spatial_distributed,
                                    ensemble_distributed=ensemble_distributed, ensemble_weights=ensemble_weights)
        self.channel_reduction, self.batch_reduction = channel_reduction, batch_reduction
        self.quadrature = GridQuadrature(grid_to_quadrature_rule(grid_type), img_shape=img_shape, crop_shape=crop_shape,
                                         crop_offset=crop_offset, normalize=True, distributed=spatial_distributed)

    @property
    def type(self):
        return LossType.Probabilistic

    def compute_counts(self, inp: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        return _compute_counts(self, inp, weight, 2)

    def combine(self, vals, counts, dim=0):
        vals, counts = _sanitize_shapes(vals, counts, dim=dim)
        return _welford_reduction_helper(vals, counts, self.batch_reduction, dim=dim)

    def finalize(self, vals, counts):
        return vals if self.batch_reduction == "mean" else vals / counts

    @torch.compiler.disable(recursive=True)
    @torch.no_grad()
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        return _reduce(self.metric_func(forecasts, observations, weight), self.channel_reduction, self.batch_reduction)


class GeometricRankHistogram(GeometricBaseMetric):
    """``functions.py:532-677``: per ``(b, c)`` the quadrature weight of the points at which ``k`` members are ``<=`` the observation,
    ``k = 0 .. E``: a trailing axis of ``E + 1`` bins"""
    _channel_dim = 2

    def __init__(self, grid_type: str, img_shape: Tuple[int, int], crop_shape: Tuple[int, int], crop_offset: Tuple[int, int],
                 normalize: Optional[bool] = False, channel_reduction: Optional[str] = "mean", batch_reduction: Optional[str] = "mean",
                 spatial_distributed: Optional[bool] = False, ensemble_distributed: Optional[bool] = False, **kwargs):
        super().__init__(grid_type=grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction, spatial_distributed=spatial_distributed)
        self.ensemble_distributed = ensemble_active(ensemble_distributed)
        # (the whole plane's weights: the ensemble-parallel path takes this rank's share of the points in forward, as CRPSLoss does)
        self.register_buffer("quad_weight_split", self.quadrature.quad_weight.reshape(1, 1, -1, 1).contiguous(), persistent=False)

    @property
    def type(self):
        return LossType.Probabilistic

    def compute_counts(self, inp: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        return super().compute_counts(inp, weight).unsqueeze(-1)

    @torch.compiler.disable(recursive=True)
    @device_guard
    def forward(self, forecasts: torch.Tensor, observations: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        sums, _ = self._ensemble_sums(forecasts, observations, weight, ENS_HIST, self.ensemble_distributed, check_weights=True)
        return _reduce(sums[..., 2:], self.channel_reduction, self.batch_reduction)
