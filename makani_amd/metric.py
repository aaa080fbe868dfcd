"""``MetricsHandler`` and its ``MetricRollout`` curves (``makani/utils/metric.py:45-740``) on the HIP path: the validation half of
the loop, with the reference's constructor arguments, handle configurations, buffers, ``update`` / ``reduce`` / ``finalize`` /
``report`` and log keys.

What the reference does per ``update`` — the ensemble mean of all channels, an index-gather copy of prediction and target per
handle, ``torch.any(torch.isnan(.))`` per handle (a host read), a mask tensor, one metric pass per handle, ``stack`` /
``combine`` / ``copy_`` per curve — is here ONE read of the planes that any handle lists and one finish launch for all handles
(``csrc/mrollout.hip``): ``mk_mrollout_sums`` forms every plane sum any handle needs (NaN targets are masked per point, the
ensemble mean lives in registers), ``mk_mrollout_finish`` forms each metric per sample in the reference's order, decides
``counts_new`` on the device and merges into row ``idt`` of the curves and counters, which are views of one flat allocation.
No step of a fused update reads the device from the host, so the update can be captured in a graph.

``update`` takes the fused pair when the inputs are on the GPU, ``E <= 32``, the "ensemble" group is not split and all handles
share one quadrature tensor (checked with ``torch.equal`` at construction); otherwise the composed per-handle path, which is
``MetricRollout.update`` on the metric classes of ``makani_amd.metrics`` exactly as the reference composes them.  Under
``spatial_distributed`` the fused path all-reduces the ``(B, J, K)`` sums once over the spatial group in front of the finish.

Deviations from the reference, stated:
  * ``scale`` is a tensor of the output channels, ``(C,)`` or ``(1, C, 1, 1)`` (default: ones).  The reference reads the files
    named in ``params`` (and loads a ``bias`` that it never uses);
  * ``logs["metrics"]["rollouts"]`` is a ``wandb.Table`` if ``wandb`` imports, otherwise ``{"columns": [...], "data": [...]}``;
  * ``save()`` raises ``NotImplementedError`` (no ``h5py``, as in ``rollout_buffer.py``); ``curves()`` returns
    ``{name: (curve_cpu, channels, lead_times)}``;
  * the ensemble mean of bf16 members is not rounded to bf16 before the deterministic sums (both paths form it in fp32);
  * the counts are formed in fp32 whatever the dtype of the members (the reference casts the weights to the members' dtype);
  * rank-histogram inputs must be finite, as in ``makani_amd.metrics``;
  * a CPU tensor raises ``RuntimeError``: there is no CPU path (construction on the CPU works: shapes, names, reports);
  * a CRPS handle with one member raises ``ValueError`` (the reference's kernel divides by ``E (E - 1)`` and dies);
  * ``finalize`` runs on the current stream (the reference uses a side stream for its reductions)."""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from . import comm as _comm
from ._lib import CONSTS, check, dtype_code, lib, prep, ptr, stream
from .ensemble import MAX_ENSEMBLE
from .metrics import (GeometricACC, GeometricCRPS, GeometricL1, GeometricRankHistogram, GeometricRMSE, GeometricSpread, GeometricSSR,
                      LossType, _bias_plane)

_BITS = {k: CONSTS["MK_MROLL_" + k] for k in ("L1", "L2", "ACC", "SPREAD", "CRPS", "HIST")}
_NSUM, _HDESC = CONSTS["MK_MROLL_NSUM"], CONSTS["MK_MROLL_HDESC"]
# metric name -> (kind of mk_mrollout_finish, the sums it needs from its planes)
_KINDS = {"L1": ("L1", _BITS["L1"]), "RMSE": ("RMSE", _BITS["L2"]), "ACC": ("ACC", _BITS["ACC"]), "CRPS": ("CRPS", _BITS["CRPS"]),
          "Spread": ("SPREAD", _BITS["SPREAD"]), "SSR": ("SSR", _BITS["SPREAD"] | _BITS["L2"]), "Rank Histogram": ("HIST", _BITS["HIST"])}
_DEFAULT_VARS = ["u10m", "t2m", "sp", "sst", "u500", "z500", "q500", "q50"]


class SimpsonQuadrature(nn.Module):
    """``functions.py:680-703``: Simpson's 1/3 rule on an even number of intervals"""

    def __init__(self, num_intervals, interval_width, device):
        super().__init__()
        weights = [0.0 for _ in range(num_intervals + 1)]
        if num_intervals % 2 != 0:
            raise NotImplementedError("Error, please specify an even number of intervals")
        for j in range(1, (num_intervals // 2 + 1)):
            weights[2 * j - 2] += 1.0
            weights[2 * j - 1] += 4.0
            weights[2 * j] += 1.0
        self.weights = torch.tensor(weights, dtype=torch.float32, device=device)
        self.weights *= interval_width / 3.0

    def forward(self, x, dim=1):
        shape = [1 for _ in range(x.dim())]
        shape[dim] = -1
        return torch.sum(x * torch.reshape(self.weights, shape), dim=dim)


class TrapezoidQuadrature(nn.Module):
    """``functions.py:706-721``"""

    def __init__(self, num_intervals, interval_width, device):
        super().__init__()
        weights = [interval_width for _ in range(num_intervals + 1)]
        weights[0] *= 0.5
        weights[-1] *= 0.5
        self.weights = torch.tensor(weights, dtype=torch.float32, device=device)

    def forward(self, x, dim=1):
        shape = [1 for _ in range(x.dim())]
        shape[dim] = -1
        return torch.sum(x * torch.reshape(self.weights, shape), dim=dim)


class Quadrature(nn.Module):
    """``functions.py:724-733``: Simpson for an even number of intervals, the trapezoid rule otherwise"""

    def __init__(self, num_intervals, interval_width, device):
        super().__init__()
        cls = SimpsonQuadrature if num_intervals % 2 == 0 else TrapezoidQuadrature
        self.quad = cls(num_intervals, interval_width, device)

    def forward(self, x, dim=1):
        return self.quad(x, dim)


def _all_gather(t, group):
    """the tensors of every rank of ``group`` (gloo moves host memory only: staged through the host there)"""
    import torch.distributed as dist
    n = dist.get_world_size(group)
    if dist.get_backend(group) == "gloo" and t.is_cuda:
        h = t.cpu()
        parts = [torch.empty_like(h) for _ in range(n)]
        dist.all_gather(parts, h, group=group)
        return [p.to(t.device) for p in parts]
    parts = [torch.empty_like(t) for _ in range(n)]
    dist.all_gather(parts, t.contiguous(), group=group)
    return parts


class MetricRollout:
    """``metric.py:45-261``: one metric's rollout curve ``(steps, channels[, aux])`` with its counter.  ``update`` composes the
    metric class as the reference does (one pass per handle, a host read for the NaN test); ``MetricsHandler`` writes the same
    buffers through the fused kernels."""

    def __init__(self, metric_name, metric_channels, metric_handle, channel_names, num_rollout_steps, dtphys, device, aux_shape=None,
                 aux_shape_finalized=None, scale=None, mask_target_nan=True, integrate=False, report_metric=True):
        self.metric_name = metric_name
        self.metric_channels = metric_channels
        self.device = torch.device(device) if isinstance(device, str) else device
        self.integrate = integrate
        self.mask_target_nan = mask_target_nan
        self.report_metric = report_metric
        self.num_rollout_steps = num_rollout_steps
        self.dtphys = dtphys
        self.aux_shape = aux_shape
        self.aux_shape_finalized = aux_shape_finalized

        self.metric_func = metric_handle().to(self.device)
        self.metric_type = self.metric_func.type
        if self.metric_func.batch_reduction == "none":
            raise ValueError("Batch reduction mode 'none' is not supported for rollout handlers")

        self.channel_mask = [channel_names.index(c) for c in metric_channels]
        if scale is not None:
            self.scale = scale[self.channel_mask].to(self.device)

        self.num_channels = len(self.metric_channels)
        if self.aux_shape is None:
            data_shape = (self.num_rollout_steps, self.num_channels)
            counter_shape = (self.num_rollout_steps, self.num_channels)
        else:
            data_shape = (self.num_rollout_steps, self.num_channels, *self.aux_shape)
            counter_shape = (self.num_rollout_steps, self.num_channels, *(1 for _ in range(len(self.aux_shape))))
        self.rollout_curve = torch.zeros(data_shape, dtype=torch.float32, device=self.device)
        self.rollout_counter = torch.zeros(counter_shape, dtype=torch.float32, device=self.device)

        pin_memory = self.device.type == "cuda"
        if self.aux_shape_finalized is None:
            data_shape_finalized = (self.num_rollout_steps, self.num_channels)
            integral_shape = self.num_channels
        else:
            data_shape_finalized = (self.num_rollout_steps, self.num_channels, *self.aux_shape_finalized)
            integral_shape = (self.num_channels, *self.aux_shape_finalized)
        self.rollout_curve_cpu = torch.zeros(data_shape_finalized, dtype=torch.float32, device="cpu", pin_memory=pin_memory)
        if self.integrate:
            self.rollout_integral = torch.zeros(integral_shape, dtype=torch.float32, device=self.device)
            self.rollout_integral_cpu = torch.zeros(integral_shape, dtype=torch.float32, device="cpu", pin_memory=pin_memory)
            self.simpquad = Quadrature(self.num_rollout_steps - 1, 1.0 / float(self.num_rollout_steps), self.device)

    @property
    def type(self):
        return self.metric_type

    def _adopt(self, curve, counter):
        """move the buffers into views of the handler's flat allocation"""
        curve.copy_(self.rollout_curve)
        counter.copy_(self.rollout_counter)
        self.rollout_curve, self.rollout_counter = curve, counter

    def zero_buffers(self):
        with torch.no_grad():
            self.rollout_curve.fill_(0.0)
            self.rollout_counter.fill_(0.0)
            if self.integrate:
                self.rollout_integral.fill_(0.0)

    @torch.no_grad()
    def update(self, inp: torch.Tensor, tar: torch.Tensor, idt: int, wgt: Optional[torch.Tensor] = None):
        if not (inp.is_cuda and tar.is_cuda):
            raise RuntimeError("makani_amd metrics run on the GPU (HIP) path only")
        inpp = inp[..., self.channel_mask, :, :]
        tarp = tar[..., self.channel_mask, :, :]
        # only mask if the target actually contains nans
        if self.mask_target_nan and torch.any(torch.isnan(tarp)):
            wgtt_nan = torch.logical_not(torch.isnan(tarp)).to(torch.float32)
            tarp = torch.where(wgtt_nan > 0.0, tarp, 0.0)
        else:
            wgtt_nan = None
        if wgt is not None:
            wgtt = wgt[..., self.channel_mask, :, :]
            if wgtt_nan is not None:
                wgtt = wgtt * wgtt_nan
        else:
            wgtt = wgtt_nan

        metric = self.metric_func(inpp, tarp, wgtt)
        if hasattr(self, "scale"):
            metric = metric * self.scale
        # (compute_counts reads shape, device and dtype of its first argument: fp32 counts whatever the dtype of the members)
        like = torch.empty_strided(inpp.shape, [0] * inpp.dim(), dtype=torch.float32, device=inpp.device)
        counts_new = self.metric_func.compute_counts(like, wgtt)

        vals = torch.stack([self.rollout_curve[idt, ...], metric], dim=0)
        counts = torch.stack([self.rollout_counter[idt, ...], counts_new.to(torch.float32)], dim=0)
        vals, counts = self.metric_func.combine(vals, counts, dim=0)
        self.rollout_curve[idt, ...].copy_(vals)
        self.rollout_counter[idt, ...].copy_(counts)

    def _combine_helper(self, vallist, countlist):
        vals = torch.stack(vallist, dim=0).contiguous()
        counts = torch.stack(countlist, dim=0).contiguous()
        for idt in range(self.num_rollout_steps):
            vtmp, ctmp = self.metric_func.combine(vals[:, idt, ...], counts[:, idt, ...], dim=0)
            self.rollout_curve[idt, ...].copy_(vtmp)
            self.rollout_counter[idt, ...].copy_(ctmp)

    def reduce(self, non_blocking=False):
        """all_gather over the "batch" group + ``combine`` per step (a group of one rank: nothing to do)"""
        with torch.no_grad():
            if _comm.get_size("batch") > 1:
                group = _comm.get_group("batch")
                self._combine_helper(_all_gather(self.rollout_curve, group), _all_gather(self.rollout_counter, group))

    def finalize(self, non_blocking=False):
        with torch.no_grad():
            rollout_curve_normalized = self.metric_func.finalize(self.rollout_curve, self.rollout_counter)
            self.rollout_curve_cpu.copy_(rollout_curve_normalized, non_blocking=non_blocking)
            if self.integrate:
                self.rollout_integral.copy_(self.simpquad(rollout_curve_normalized, dim=0))
                self.rollout_integral_cpu.copy_(self.rollout_integral, non_blocking=non_blocking)

    def report(self, index=0, table=False):
        log = {}
        if self.report_metric:
            rollout_curve_arr = self.rollout_curve_cpu.numpy()
            for idx, var_name in enumerate(self.metric_channels):
                log[f"{self.metric_name} {var_name}({(index+1) * self.dtphys})"] = rollout_curve_arr[index, idx]
            if self.integrate:
                rollout_integral_arr = self.rollout_integral_cpu.numpy()
                for idx, var_name in enumerate(self.metric_channels):
                    log[f"{self.metric_name} AUC {var_name}({self.num_rollout_steps * self.dtphys})"] = rollout_integral_arr[idx]
        report = log
        if table:
            if self.report_metric:
                table_data = []
                for d in range(0, self.num_rollout_steps):
                    for idx, var_name in enumerate(self.metric_channels):
                        table_data.append([self.metric_name, var_name, (d + 1) * self.dtphys, rollout_curve_arr[d, idx]])
                report = (log, table_data)
            else:
                report = (log, [])
        return report


class MetricsHandler:
    """``metric.py:264-746``.  ``params`` supplies ``channel_names``, ``dt``, ``dhours``, ``split_data_channels``,
    ``img_shape_x_resampled`` / ``img_shape_y_resampled``, ``img_crop_offset_x`` / ``img_crop_offset_y`` and, through ``get``,
    ``model_grid_type``, ``ensemble_size``, ``log_to_screen`` and ``log_to_wandb``; ``climatology`` is ``(1, C, H, W)`` over all
    of ``channel_names`` (normalised with bias and scale) or None.  See the module docstring for ``scale`` and the other stated
    deviations, and for which path ``update`` takes."""

    def __init__(self, params, climatology, num_rollout_steps, device, l1_var_names=_DEFAULT_VARS, rmse_var_names=_DEFAULT_VARS,
                 acc_var_names=_DEFAULT_VARS, crps_var_names=_DEFAULT_VARS, spread_var_names=_DEFAULT_VARS, ssr_var_names=_DEFAULT_VARS,
                 rh_var_names=[], mask_target_nan=True, wb2_compatible=False, scale=None):
        self.device = torch.device(device) if isinstance(device, str) else device
        self.log_to_screen = params.get("log_to_screen", False)
        self.log_to_wandb = params.get("log_to_wandb", False)
        self.channel_names = params.channel_names
        _comm.autodetect()
        self.spatial_distributed = _comm.is_distributed("spatial") and (_comm.get_size("spatial") > 1)
        self.ensemble_distributed = _comm.is_distributed("ensemble") and (_comm.get_size("ensemble") > 1)

        self.dtxdh = params.dt * params.dhours
        self.dd = 24 // self.dtxdh

        def present(names):
            return [x for x in names if x in self.channel_names]

        self.l1_var_names, self.rmse_var_names, self.acc_var_names = present(l1_var_names), present(rmse_var_names), present(acc_var_names)
        self.crps_var_names, self.spread_var_names = present(crps_var_names), present(spread_var_names)
        self.ssr_var_names, self.rh_var_names = present(ssr_var_names), present(rh_var_names)

        self.split_data_channels = params.get("split_data_channels", False)
        if self.split_data_channels:
            raise NotImplementedError("Error, split_data_channels is not supported")

        nchan = len(self.channel_names)
        if scale is None:
            scale = torch.ones(nchan, dtype=torch.float32)
        scale = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
        if scale.numel() != nchan:
            raise ValueError(f"scale holds {scale.numel()} entries for {nchan} output channels")

        self.num_rollout_steps = num_rollout_steps
        self.img_shape = (params.img_shape_x_resampled, params.img_shape_y_resampled)
        self.crop_shape = (params.img_shape_x_resampled, params.img_shape_y_resampled)
        self.crop_offset = (params.get("img_crop_offset_x", 0), params.get("img_crop_offset_y", 0))
        grid_type = params.get("model_grid_type", "equiangular")
        self.mask_target_nan = mask_target_nan
        if wb2_compatible:
            if grid_type == "equiangular":
                grid_type = "weatherbench2"
            else:
                raise ValueError(f"weatherbench2 compatibility only supported on equiangular grids. Got {grid_type} instead")

        common = dict(grid_type=grid_type, img_shape=self.img_shape, crop_shape=self.crop_shape, crop_offset=self.crop_offset,
                      normalize=True, channel_reduction="none", batch_reduction="sum", spatial_distributed=self.spatial_distributed)
        ens = dict(common, ensemble_distributed=self.ensemble_distributed)
        self.metric_handles = []

        def add(name, channels, handle, **kw):
            self.metric_handles.append(MetricRollout(metric_name=name, metric_channels=channels, metric_handle=handle,
                                                     channel_names=self.channel_names, num_rollout_steps=self.num_rollout_steps,
                                                     dtphys=self.dtxdh, device=self.device, mask_target_nan=self.mask_target_nan, **kw))

        if self.l1_var_names:
            add("L1", self.l1_var_names, partial(GeometricL1, **common), integrate=False, report_metric=True)
        if self.rmse_var_names:
            add("RMSE", self.rmse_var_names, partial(GeometricRMSE, **common), scale=scale, integrate=False, report_metric=True)
        if self.acc_var_names:
            # important: the climatology is assumed to be normalized with bias and scale
            if climatology is not None:
                channel_mask = [self.channel_names.index(c) for c in self.acc_var_names]
                clim = climatology.to(torch.float32)[:, channel_mask, ...].contiguous().to(self.device)
            else:
                clim = None
            add("ACC", self.acc_var_names, partial(GeometricACC, method="macro", bias=clim, **common), integrate=True, report_metric=True)
        if self.crps_var_names:
            add("CRPS", self.crps_var_names, partial(GeometricCRPS, crps_type="skillspread", **ens), scale=scale, integrate=False,
                report_metric=True)
        if self.spread_var_names:
            add("Spread", self.spread_var_names, partial(GeometricSpread, **ens), scale=scale, integrate=False, report_metric=True)
        if self.ssr_var_names:
            add("SSR", self.ssr_var_names, partial(GeometricSSR, **ens), integrate=False, report_metric=True)
        if self.rh_var_names:
            ens_size = params.get("ensemble_size", 1)
            add("Rank Histogram", self.rh_var_names, partial(GeometricRankHistogram, **ens), aux_shape=(ens_size + 1,),
                aux_shape_finalized=(ens_size + 1,), integrate=False, report_metric=False)

        if _comm.get_size("spatial") > 1:
            from . import distributed as thd
            self.gather_shapes_h = thd.compute_split_shapes(self.crop_shape[0], _comm.get_size("h"))
            self.gather_shapes_w = thd.compute_split_shapes(self.crop_shape[1], _comm.get_size("w"))
        self.use_fused = True          # False: every update takes the composed per-handle path
        self._plan()

    # ---- the flat allocation and the device tables of the fused path ---------------------------------------------------------
    def _plan(self):
        """One flat device allocation for all curves and counters (the handles' buffers become views of it), and the tables of
        ``mk_mrollout_sums`` / ``mk_mrollout_finish``: the planes = the union of the listed channels in order of first
        appearance, the bits of the sums any handle needs from each, the climatology row of ACC's planes."""
        handles = self.metric_handles
        total = sum(h.rollout_curve.numel() + h.rollout_counter.numel() for h in handles)
        self._flat = torch.zeros(max(total, 1), dtype=torch.float32, device=self.device)
        planes, bits, crow = [], {}, {}
        hdesc, hplanes, hscale, at = [], [], [], 0
        for h in handles:
            kind, need = _KINDS[h.metric_name]
            nc, nv = h.rollout_curve.numel(), h.rollout_counter.numel()
            h._adopt(self._flat[at:at + nc].view(h.rollout_curve.shape), self._flat[at + nc:at + nc + nv].view(h.rollout_counter.shape))
            hdesc.append([CONSTS["MK_MROLL_KIND_" + kind], h.num_channels, len(hplanes), at, at + nc, self.num_rollout_steps])
            at += nc + nv
            for i, c in enumerate(h.channel_mask):
                if c not in bits:
                    planes.append(c)
                    bits[c] = 0
                bits[c] |= need
                if h.metric_name == "ACC" and getattr(h.metric_func, "bias", None) is not None:
                    crow[c] = i
                hplanes.append(planes.index(c))
            hscale += (h.scale.reshape(-1).tolist() if hasattr(h, "scale") else [1.0] * h.num_channels)
        for name in ("rmse", "acc", "crps", "ssr", "rh"):
            full = {"rmse": "RMSE", "acc": "ACC", "crps": "CRPS", "ssr": "SSR", "rh": "Rank Histogram"}[name]
            for h in handles:
                if h.metric_name == full:
                    setattr(self, name + "_curve", h.rollout_curve)
        self._by_name = {h.metric_name: h for h in handles}
        self._J = len(planes)
        quads = [h.metric_func.quadrature.quad_weight for h in handles]
        self._shared_quadrature = bool(handles) and all(torch.equal(q, quads[0]) for q in quads)
        self._acc_eps = getattr(self._by_name["ACC"].metric_func, "eps", 1e-8) if "ACC" in self._by_name else 1e-8
        self._ssr_eps = getattr(self._by_name["SSR"].metric_func, "eps", 1e-6) if "SSR" in self._by_name else 1e-6
        if self.device.type != "cuda" or not handles:
            return
        dev = self.device
        self._table = torch.tensor([[c, bits[c], crow.get(c, -1)] for c in planes], dtype=torch.int32, device=dev)
        self._hdesc = torch.tensor(hdesc, dtype=torch.int32, device=dev)
        self._hplanes = torch.tensor(hplanes, dtype=torch.int32, device=dev)
        self._hscale = torch.tensor(hscale, dtype=torch.float32, device=dev)
        self._quad = quads[0].reshape(-1).contiguous()
        self._clim = None
        if crow:
            f = self._by_name["ACC"].metric_func
            self._clim = _bias_plane(f.bias, len(self.acc_var_names), *self._quad_shape(quads[0]))

    @staticmethod
    def _quad_shape(q):
        return tuple(q.shape[-2:])

    # ---- the reference's interface ------------------------------------------------------------------------------------------
    def _gather_input(self, x: torch.Tensor) -> torch.Tensor:
        """gather the lat/lon shards of ``x`` over the "h" and "w" groups"""
        for name, dim, attr in (("h", -2, "gather_shapes_h"), ("w", -1, "gather_shapes_w")):
            if _comm.get_size(name) > 1:
                shapes = getattr(self, attr)
                pad = max(shapes) - x.shape[dim]
                xp = torch.nn.functional.pad(x, (0, pad) if dim == -1 else (0, 0, 0, pad)) if pad else x
                parts = _all_gather(xp.contiguous(), _comm.get_group(name))
                x = torch.cat([p.narrow(dim, 0, s) for p, s in zip(parts, shapes)], dim=dim)
        return x

    def initialize_buffers(self):
        self.valid_buffer = torch.zeros((2), dtype=torch.float32, device=self.device)
        self.valid_loss = self.valid_buffer[0].view(-1)
        self.valid_steps = self.valid_buffer[1].view(-1)

    def zero_buffers(self):
        with torch.no_grad():
            self.valid_buffer.fill_(0)
        for handle in self.metric_handles:
            handle.zero_buffers()

    def _fused(self, prediction, E):
        return (self.use_fused and prediction.is_cuda and self.device.type == "cuda" and E <= MAX_ENSEMBLE and not self.ensemble_distributed
                and self._shared_quadrature)

    @torch.no_grad()
    def update(self, prediction, target, loss, idt, weight=None):
        """update the buffers on rollout step ``idt``: prediction ``(B, C, H, W)`` or ``(B, E, C, H, W)``, target ``(B, C, H, W)``,
        weight None or broadcastable to the target"""
        E = prediction.shape[1] if prediction.dim() == 5 else 1
        if "CRPS" in self._by_name and E == 1 and not self.ensemble_distributed:
            raise ValueError("the CRPS handle needs an ensemble of at least two members (pass crps_var_names=[] for a deterministic model)")
        if not (prediction.is_cuda and target.is_cuda):
            raise RuntimeError("makani_amd metrics run on the GPU (HIP) path only")
        if not 0 <= idt < self.num_rollout_steps:
            raise IndexError(f"rollout step {idt} outside the {self.num_rollout_steps} steps of the curves")
        if "Rank Histogram" in self._by_name and not self.ensemble_distributed and self.rh_curve.shape[-1] != E + 1:
            raise ValueError(f"the rank histogram was built for ensemble_size = {self.rh_curve.shape[-1] - 1}, the prediction holds {E} members")
        if self._fused(prediction, E):
            with torch.cuda.device(prediction.device):
                self._update_fused(prediction, target, idt, weight, E)
        else:
            self._update_composed(prediction, target, idt, weight)
        if idt == 0:
            self.valid_steps += 1.0
            self.valid_loss += loss

    def _update_composed(self, prediction, target, idt, weight):
        if prediction.dim() == 5:
            prediction_mean = torch.mean(prediction, dim=1, dtype=torch.float32)          # (fp32 sum and result, no fp32 copy of the members)
            if self.ensemble_distributed:
                from . import ops
                ops._all_reduce_sum(prediction_mean, _comm.get_group("ensemble"))
                prediction_mean = prediction_mean / float(_comm.get_size("ensemble"))
        else:
            prediction_mean = prediction
            prediction = prediction.unsqueeze(1)
        for handle in self.metric_handles:
            if handle.type == LossType.Deterministic:
                handle.update(prediction_mean, target, idt, weight)
            elif handle.type == LossType.Probabilistic:
                handle.update(prediction, target, idt, weight)
            else:
                raise NotImplementedError(f"Error, LossType {handle.type} not implemented.")

    def _update_fused(self, prediction, target, idt, weight, E):
        B, C, H, W = target.shape
        N = H * W
        if prediction.shape[-3:] != target.shape[-3:] or prediction.shape[0] != B:
            raise ValueError(f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)} do not match")
        if C != len(self.channel_names):
            raise ValueError(f"the inputs hold {C} channels, channel_names lists {len(self.channel_names)}")
        if self._quad.numel() != N:
            raise ValueError(f"the quadrature holds {self._quad.numel()} weights for planes of {H} x {W} points")
        pred, tar = prep(prediction), prep(target)
        w = weight.float().expand(B, C, H, W).contiguous() if weight is not None else None
        L = lib()
        J, K = self._J, _NSUM + E + 1
        chunks = L.mk_metric_chunks(N)
        partial_ = torch.empty((B * J * chunks * K,), dtype=torch.float32, device=pred.device)
        sums = torch.empty((B, J, K), dtype=torch.float32, device=pred.device) if self.spatial_distributed else None
        ja = self._clim.shape[0] if self._clim is not None else 0
        check(L.mk_mrollout_sums(ptr(pred), dtype_code(pred), ptr(tar), dtype_code(tar), ptr(w), ptr(self._quad), ptr(self._clim),
                                 ptr(self._table), ptr(partial_), ptr(sums), B, E, C, J, ja, N, int(bool(self.mask_target_nan)), stream()),
              "mk_mrollout_sums")
        if sums is not None:          # ONE all-reduce of the (B, J, K) sums over the spatial group
            from . import distributed as thd
            sums = thd.reduce_from_spatial_region(sums).contiguous()
            partial_, chunks = sums, 1
        check(L.mk_mrollout_finish(ptr(partial_), chunks, ptr(self._hdesc), ptr(self._hplanes), ptr(self._hscale), ptr(self._flat),
                                   self._flat.numel(), len(self.metric_handles), B, E, J, int(idt), int(weight is not None),
                                   float(self._acc_eps), float(self._ssr_eps), stream()), "mk_mrollout_finish")

    def finalize(self):
        """reduce over the "batch" group, normalise the curves, copy them to the host and assemble the reference's ``logs``"""
        import torch.distributed as dist
        with torch.no_grad():
            if dist.is_available() and dist.is_initialized() and _comm.get_size("batch") > 1:
                from . import ops
                ops._all_reduce_sum(self.valid_buffer, _comm.get_group("batch"))
            for handle in self.metric_handles:
                handle.reduce(non_blocking=True)
            self.valid_loss /= self.valid_steps
            for handle in self.metric_handles:
                handle.finalize(non_blocking=True)
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)

            valid_loss = self.valid_loss.item()
            valid_steps = self.valid_steps.item()
            logs = {"base": {"validation steps": valid_steps, "validation loss": valid_loss}, "metrics": {}}
            table_data = []
            for handle in self.metric_handles:
                if handle.metric_name != "ACC":
                    tmplog = handle.report(index=0, table=False)
                    for key in tmplog:
                        logs["metrics"]["validation " + key] = tmplog[key]
                tmplog, tmptable = handle.report(index=self.num_rollout_steps - 1, table=True)
                for key in tmplog:
                    logs["metrics"]["validation " + key] = tmplog[key]
                table_data += tmptable
            columns = ["metric type", "variable name", "time [h]", "value"]
            try:
                import wandb
                logs["metrics"]["rollouts"] = wandb.Table(data=table_data, columns=columns)
            except ImportError:
                logs["metrics"]["rollouts"] = {"columns": columns, "data": table_data}
        self.logs = logs
        return logs

    def curves(self):
        """``{metric name: (finalized curve on the host, channels, lead times)}`` — what the reference's ``save`` writes"""
        return {h.metric_name: (h.rollout_curve_cpu, list(h.metric_channels), h.dtphys * torch.arange(1, h.num_rollout_steps + 1))
                for h in self.metric_handles}

    def save(self, metrics_file: str):
        raise NotImplementedError("the HDF5 writer of the metrics is not part of the HIP path: curves() returns what it would write")
