"""Online rollout diagnostics on the HIP path: the running mean and standard deviation per lead time of the de-normalised
fields, of their angular power spectrum and of their latitude-weighted longitude spectrum — ``MeanStdBuffer``,
``TemporalAverageBuffer``, ``SpectrumAverageBuffer`` and ``ZonalSpectrumAverageBuffer`` of
``makani/utils/inference/rollout_buffer.py:670-1338`` with their constructor arguments, attributes, ``zero_buffers`` /
``update`` / ``finalize`` and the Welford state ``running_mean`` / ``running_var`` (= M2) / ``num_samples_tracked``.

What an ``update`` launches (``csrc/rollout.hip``):

* temporal: ONE kernel (``mk_welford_update``).  The batch is read in place through the channel list, ``scale * x + bias`` and
  the batch statistics live in registers, the running pair is read and written once.
* spectrum: ``RealSHT.analysis`` of truth and of the members (two calls, no ``torch.cat``), ``mk_power_spectrum`` on the
  S-layout coefficients of each into ONE ``(B, C, E1, L)`` tensor in the reference's post-permute order, then
  ``mk_welford_update`` on it.  Scale and bias are applied to the COEFFICIENTS (the transform is linear: the bias only moves
  order 0, by ``bias * one[l]`` with ``one`` the transform of the constant field 1, formed in fp64 from the quadrature and the
  Legendre functions of ``legendre.py``); no ``scale * x + bias`` field, no ``|c|^2`` tensor and no permuted copy exist.
  Under a "w" split the ``(B, C, E1, L_loc)`` sums are added over the "w" group before the statistics.
* zonal: ``ops.rfft_rows`` (``norm="forward"``) of truth and of the members and ``mk_zonal_welford`` on each, which forms the
  weighted powers, their batch statistics and the merge in one pass and turns (rows x orders) tiles in LDS.

The sample count stays in device memory: the kernels read it, ``update`` adds the batch size behind them on the same stream.
No ``update`` reads a device value on the host, so it can be captured in a graph and replayed.

Deviations from the reference:

* No HDF5 writer (``h5py`` / ``mpi4py``): ``output_file is not None`` raises ``NotImplementedError`` at construction,
  ``_write_output_data`` and the field dumper ``RolloutBuffer`` are not provided.  ``finalize()`` RETURNS ``(mean, std)``.
* A CPU tensor raises ``RuntimeError``: there is no CPU path.
* ``ZonalSpectrumAverageBuffer`` with a split "w" group raises ``NotImplementedError`` (it needs a distributed planar FFT,
  which this package does not have); the "h" split is supported.
* When ``output_channels`` is not all channels in order, the spectral buffers gather the selected planes once with
  ``index_select`` in front of the transform; with the identity selection nothing is copied.  The temporal buffer reads the
  selected planes in place in either case.
* For bfloat16 input the spectra are rounded to bfloat16 before the statistics (``spect.to(dtype)`` with the input's dtype);
  the transform reads the bfloat16 values and works in fp32.
* ``targ`` may be ``(B, 1, C, H, W)`` as in the reference or ``(B, C, H, W)``.
"""
import math
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import comm
from . import legendre as _leg
from . import ops
from ._lib import check, dtype_code, lib, need_gpu, prep, ptr, stream

__all__ = ["MeanStdBuffer", "TemporalAverageBuffer", "SpectrumAverageBuffer", "ZonalSpectrumAverageBuffer", "power_spectrum"]


def constant_field_coefficients(sht) -> np.ndarray:
    """``one[l]`` (fp64, all ``sht.lmax`` degrees): the order-0 coefficients of the constant field 1 under ``sht`` =
    ``2 pi sum_k w_k P_l^0(theta_k)``.  ``sqrt(4 pi)`` at l = 0; the other degrees are whatever the quadrature leaves of them
    (rounding noise where the rule integrates degree l exactly, as Gauss-Legendre and Clenshaw-Curtis do below ``nlat``; more
    for a truncated ``lmax`` beyond that or another rule), so the kernel is handed the whole row and not a delta."""
    theta, wq = _leg.colatitudes(sht.nlat, sht.grid)
    P0 = _leg.legendre_matrix(1, sht.lmax, theta, norm=sht.norm, inverse=False, csphase=sht.csphase)[0]      # (lmax, nlat)
    return 2.0 * math.pi * (P0 * wq[None, :]).sum(axis=1)


def _one(sht, device) -> torch.Tensor:
    """this shard's slice of ``one`` as an fp32 device tensor (rounded once), cached on the transform"""
    cache = sht.__dict__.setdefault("_mk_one", {})
    key = str(device)
    if key not in cache:
        l_off = getattr(sht, "l_off", 0)
        l_loc = sht.l_shapes[sht.comm_rank_polar] if hasattr(sht, "l_shapes") else sht.lmax
        full = constant_field_coefficients(sht)
        cache[key] = torch.from_numpy(full[l_off:l_off + l_loc].astype(np.float32)).to(device)
    return cache[key]


def _shard(sht):
    """(l_off, m_off) of the coefficients ``sht.analysis`` returns"""
    return getattr(sht, "l_off", 0), getattr(sht, "m_off", 0)


def _spectrum_into(out, x4, sht, scale, bias, B, E, e0):
    """``x4`` (B * E, C, H, W) -> ``out[:, :, e0:e0 + E, :]`` of (B, C, E1, L): one analysis, one launch"""
    C = x4.shape[1]
    S = sht.analysis(x4)
    L, M, _, R = S.shape
    l_off, m_off = _shard(sht)
    check(lib().mk_power_spectrum(ptr(S), ptr(scale), ptr(bias), ptr(_one(sht, x4.device)) if bias is not None else None, ptr(out),
                                  dtype_code(out), L, M, R, ops.round4(C), B, E, C, out.shape[2], e0, l_off - m_off, m_off, stream()),
          "mk_power_spectrum")


def _vec(v, C, device, what):
    if v is None:
        return None
    v = torch.as_tensor(v, dtype=torch.float32, device=device).reshape(-1).contiguous()
    if v.numel() != C:
        raise ValueError(f"{what} has {v.numel()} entries for {C} channels")
    return v


@torch.no_grad()
def power_spectrum(x: torch.Tensor, sht, scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Angular power spectrum of ``scale * x + bias``: ``x`` (..., C, H, W) float32 | bfloat16 -> (..., C, L) float32 with
    ``out[..., c, l] = sum_m c_m |sht(scale_c x_c + bias_c)[l, m]|^2``, ``c_m`` = 1 for m = 0 and 2 otherwise.  ``sht``: a
    ``RealSHT`` or ``DistributedRealSHT`` of this package; with the latter ``x`` is the local shard, L the local degrees and
    the sums are this rank's orders only (add them over the "w" group).  ``scale`` / ``bias``: per channel, optional."""
    need_gpu(x, "rollout diagnostics")
    if x.dim() < 3:
        raise ValueError(f"expected (..., C, H, W), got {tuple(x.shape)}")
    lead, C = x.shape[:-3], x.shape[-3]
    x4 = prep(x).reshape(-1, C, *x.shape[-2:])
    with torch.cuda.device(x.device):
        l_loc = _one(sht, x.device).numel()
        out = torch.empty((x4.shape[0], C, 1, l_loc), dtype=torch.float32, device=x.device)
        _spectrum_into(out, x4, sht, _vec(scale, C, x.device, "scale"), _vec(bias, C, x.device, "bias"), x4.shape[0], 1, 0)
    return out.reshape(*lead, C, l_loc)


class MeanStdBuffer:
    """Welford state per lead time (``rollout_buffer.py:670-783``): ``running_mean`` / ``running_var`` (the centred sum of
    squares M2) of shape ``(num_rollout_steps, C, *variable_shape)`` fp32 and ``num_samples_tracked`` int64, all on the device."""

    def __init__(self, num_rollout_steps: int, rollout_dt: int, variable_shape: Union[Tuple[int], Tuple[int, int]],
                 channel_names: List[str], device: Union[str, torch.device], scale: Optional[torch.Tensor] = None,
                 bias: Optional[torch.Tensor] = None, output_channels: List[str] = [], output_file: Optional[str] = None):
        self.num_rollout_steps = num_rollout_steps
        self.rollout_dt = rollout_dt
        self.output_channels = output_channels
        self.output_file = output_file
        self.channel_mask = [channel_names.index(c) for c in self.output_channels]
        self.num_channels = len(self.output_channels)
        if not self.num_channels > 0:
            raise ValueError(f"Empty channel lists aren't suported. Got {self.output_channels}.")
        if output_file is not None:
            raise NotImplementedError("the HDF5 writer of the rollout diagnostics is not part of the HIP path: finalize() returns (mean, std)")
        self.device = torch.device(device) if isinstance(device, str) else device
        self.num_source_channels = len(channel_names)
        self._identity = self.channel_mask == list(range(self.num_source_channels))
        self._has_scale, self._has_bias = scale is not None, bias is not None
        if scale is not None:
            self.scale = scale.squeeze()[self.channel_mask].to(self.device, torch.float32)
        else:
            self.scale = torch.ones(self.num_channels, device=self.device)
        if bias is not None:
            self.bias = bias.squeeze()[self.channel_mask].to(self.device, torch.float32)
        else:
            self.bias = torch.zeros(self.num_channels, device=self.device)
        # what the kernels read: flat per-channel rows (None: identity, nothing is multiplied or added)
        self._scale = self.scale.reshape(-1).contiguous() if self._has_scale else None
        self._bias = self.bias.reshape(-1).contiguous() if self._has_bias else None
        self._chan = None if self._identity else torch.tensor(self.channel_mask, dtype=torch.int32, device=self.device)
        self._chan_long = None if self._identity else torch.tensor(self.channel_mask, dtype=torch.int64, device=self.device)

        size = (self.num_rollout_steps, self.num_channels, *variable_shape)
        self.running_mean = torch.zeros(size, dtype=torch.float32, device=self.device)
        self.running_var = torch.zeros(size, dtype=torch.float32, device=self.device)
        self.variable_dims = len(variable_shape)
        self.num_samples_tracked = torch.zeros((self.num_rollout_steps, 1, *(1 for _ in range(self.variable_dims))), dtype=torch.int64,
                                               device=self.device)

    def zero_buffers(self):
        with torch.no_grad():
            self.running_mean.fill_(0.0)
            self.running_var.fill_(0.0)
            self.num_samples_tracked.fill_(0)

    def _check_step(self, idt):
        if not 0 <= int(idt) < self.num_rollout_steps:
            raise IndexError(f"lead time index {idt} outside [0, {self.num_rollout_steps})")

    def _welford(self, src, idt, chan=None, scale=None, bias=None, channels=1):
        """``src`` (B, Csrc, N) f32 | bf16 merged into slot ``idt`` seen as (channels, N); the count is not advanced"""
        B, Csrc, N = src.shape
        check(lib().mk_welford_update(ptr(src), dtype_code(src), ptr(chan), ptr(scale), ptr(bias), ptr(self.running_mean[idt]),
                                      ptr(self.running_var[idt]), ptr(self.num_samples_tracked[idt]), B, Csrc, channels, N, stream()),
              "mk_welford_update")

    def _advance(self, idt, B):
        self.num_samples_tracked[idt] += B                    # a device add behind the kernels on the same stream

    def _select(self, x, dim):
        if x.shape[dim] != self.num_source_channels:
            raise ValueError(f"expected {self.num_source_channels} channels in dim {dim}, got {tuple(x.shape)}")
        return x if self._identity else x.index_select(dim, self._chan_long)

    def _aggregate_stats(self, group_name="data"):
        """pool the states of the ranks of a group (``:755-783``): n = sum n_k, mean = sum n_k mean_k / n,
        M2 = sum M2_k + sum n_k (mean_k - mean)^2.  Plain torch on the state tensors."""
        if comm.get_size(group_name) > 1:
            group = comm.get_group(group_name)
            with torch.no_grad():
                counts_old = self.num_samples_tracked.clone()
                means_old = self.running_mean.clone()
                counts_agg = counts_old.clone()
                ops._all_reduce_sum(counts_agg, group)
                means_agg = counts_old * means_old / counts_agg.to(dtype=torch.float32)      # normalised before the sum
                ops._all_reduce_sum(means_agg, group)
                m2s_agg = self.running_var.clone()
                ops._all_reduce_sum(m2s_agg, group)
                deltas = torch.square(means_old - means_agg) * counts_old
                ops._all_reduce_sum(deltas, group)
                m2s_agg += deltas
                self.num_samples_tracked[...] = counts_agg
                self.running_mean[...] = means_agg
                self.running_var[...] = m2s_agg

    def _finalize(self, group_name):
        self._aggregate_stats(group_name)
        std = torch.sqrt(self.running_var / (self.num_samples_tracked.to(dtype=torch.float32) - 1.0))
        return self.running_mean, std


class TemporalAverageBuffer(MeanStdBuffer):
    """Running mean / standard deviation per lead time and grid point of ``scale * data + bias`` (``:786-949``).
    ``update(data (B, len(channel_names), H_loc, W_loc), idt)``; ``finalize() -> (mean, std)`` of shape (T, C, H_loc, W_loc), pooled
    over the "data" group."""

    def __init__(self, num_rollout_steps: int, rollout_dt: int, img_shape: Tuple[int, int], local_shape: Tuple[int, int],
                 local_offset: Tuple[int, int], channel_names: List[str], lat_lon: Tuple[List[float], List[float]],
                 device: Union[str, torch.device], scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 output_channels: List[str] = [], output_file: Optional[str] = None):
        super().__init__(num_rollout_steps=num_rollout_steps, rollout_dt=rollout_dt, variable_shape=tuple(local_shape),
                         channel_names=channel_names, device=device, scale=scale, bias=bias, output_channels=output_channels,
                         output_file=output_file)
        self.img_shape, self.local_shape, self.local_offset, self.lat_lon = img_shape, local_shape, local_offset, lat_lon
        self.bias = self.bias.reshape(1, -1, 1, 1)
        self.scale = self.scale.reshape(1, -1, 1, 1)

    @torch.no_grad()
    def update(self, data: torch.Tensor, idt: int):
        need_gpu(data, "rollout diagnostics")
        self._check_step(idt)
        if data.dim() != 4 or data.shape[1] != self.num_source_channels or tuple(data.shape[2:]) != tuple(self.local_shape):
            raise ValueError(f"expected (B, {self.num_source_channels}, {self.local_shape[0]}, {self.local_shape[1]}), got {tuple(data.shape)}")
        x = prep(data)
        B, Csrc = x.shape[:2]
        with torch.cuda.device(x.device):
            self._welford(x.view(B, Csrc, -1), idt, self._chan, self._scale, self._bias, channels=self.num_channels)
            self._advance(idt, B)

    def finalize(self):
        return self._finalize("data")


class _SpectralBuffer(MeanStdBuffer):
    """what the two spectral buffers share: the member axis and the split of truth and members"""

    def _members(self, ensemble_size):
        self.ensemble_size = ensemble_size
        self._truth = comm.get_rank("ensemble") == 0
        return ensemble_size + (1 if self._truth else 0)

    def _sources(self, data, targ):
        """[(x4 (B * E, C, H, W), E, e0)] for truth (ensemble rank 0 only) and members; the selected channels"""
        need_gpu(data, "rollout diagnostics")
        if data.dim() != 5 or data.shape[1] != self.ensemble_size:
            raise ValueError(f"expected data (B, {self.ensemble_size}, C, H, W), got {tuple(data.shape)}")
        B = data.shape[0]
        out = []
        if self._truth:
            need_gpu(targ, "rollout diagnostics")
            if targ.dim() == 5:
                if targ.shape[1] != 1:
                    raise ValueError(f"expected targ (B, 1, C, H, W) or (B, C, H, W), got {tuple(targ.shape)}")
                targ = targ[:, 0]
            if targ.shape[0] != B or targ.dtype != data.dtype:
                raise ValueError("targ and data differ in batch size or dtype")
            out.append((prep(self._select(targ, 1)), 1, 0))
        d = prep(self._select(data, 2))
        out.append((d.reshape(B * self.ensemble_size, *d.shape[2:]), self.ensemble_size, 1 if self._truth else 0))
        return B, out

    def finalize(self):
        return self._finalize("batch")


class SpectrumAverageBuffer(_SpectralBuffer):
    """Running mean / standard deviation per lead time of the angular power spectrum of truth and members (``:952-1097``).
    ``update(data (B, E, C, H, W), targ (B, 1, C, H, W), idt)``; state (T, C, E1, L_loc), E1 = E + 1 on ensemble rank 0 (truth is
    member 0 there) and E otherwise; ``finalize() -> (mean, std)``, pooled over the "batch" group.  ``spatial_distributed``:
    local fields in, this "h" rank's degrees out, every "w" rank of a row holding the same state."""

    def __init__(self, num_rollout_steps: int, rollout_dt: int, img_shape: Tuple[int, int], ensemble_size: int, grid_type: str,
                 channel_names: List[str], device: Union[str, torch.device], scale: Optional[torch.Tensor] = None,
                 bias: Optional[torch.Tensor] = None, output_channels: List[str] = [], output_file: Optional[str] = None,
                 spatial_distributed: Optional[bool] = False):
        from . import distributed as thd
        from .sht import RealSHT
        self.spatial_distributed = spatial_distributed
        if spatial_distributed and thd.ensure_initialized():
            self.sht = thd.DistributedRealSHT(*img_shape, grid=grid_type)
            self.lmax = self.sht.lmax
            self.lmax_local = self.sht.l_shapes[self.sht.comm_rank_polar]
            self.lmax_offset = self.sht.l_off
            self._w_group = thd.azimuth_group() if thd.azimuth_group_size() > 1 else None
        else:
            self.sht = RealSHT(*img_shape, grid=grid_type)
            self.lmax = self.sht.lmax
            self.lmax_local = self.lmax
            self.lmax_offset = 0
            self._w_group = None
        enssize = self._members(ensemble_size)
        super().__init__(num_rollout_steps=num_rollout_steps, rollout_dt=rollout_dt, variable_shape=(enssize, self.lmax_local),
                         channel_names=channel_names, device=device, scale=scale, bias=bias, output_channels=output_channels,
                         output_file=output_file)
        self.img_shape = img_shape
        self.sht = self.sht.to(self.device)
        self.bias = self.bias.reshape(1, 1, -1, 1, 1)
        self.scale = self.scale.reshape(1, 1, -1, 1, 1)

    @torch.no_grad()
    def update(self, data: torch.Tensor, targ: torch.Tensor, idt: int):
        self._check_step(idt)
        B, sources = self._sources(data, targ)
        E1 = self.running_mean.shape[2]
        with torch.cuda.device(data.device):
            # the sums over the local orders stay fp32 until the "w" ranks have added theirs
            dt = torch.float32 if self._w_group is not None else data.dtype
            spect = torch.empty((B, self.num_channels, E1, self.lmax_local), dtype=dt, device=data.device)
            for x4, E, e0 in sources:
                _spectrum_into(spect, x4, self.sht, self._scale, self._bias, B, E, e0)
            if self._w_group is not None:
                ops._all_reduce_sum(spect, self._w_group)
                spect = spect.to(data.dtype)
            self._welford(spect.view(B, 1, -1), idt)
            self._advance(idt, B)


class ZonalSpectrumAverageBuffer(_SpectralBuffer):
    """Running mean / standard deviation per lead time of ``cos(lat) |rfft(x, norm="forward")|^2``, orders m >= 1 doubled
    (``:1176-1338``).  ``update(data (B, E, C, H_loc, W), targ, idt)``; state (T, C, E1, nlat_loc, mmax); ``finalize() -> (mean, std)``,
    pooled over the "batch" group.  ``spatial_distributed``: the latitudes may be split over "h"; a split "w" group is refused."""

    def __init__(self, num_rollout_steps: int, rollout_dt: int, img_shape: Tuple[int, int], ensemble_size: int,
                 channel_names: List[str], lat_lon: Tuple[List[float], List[float]], device: Union[str, torch.device],
                 scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, output_channels: List[str] = [],
                 output_file: Optional[str] = None, spatial_distributed: Optional[bool] = False):
        from . import distributed as thd
        if spatial_distributed:
            comm.autodetect()
        self.spatial_distributed = bool(spatial_distributed) and comm.get_size("spatial") > 1
        self.nlat, self.nlon = img_shape
        _leg.factorize_half(self.nlon)                        # raises for a longitude count the FFT does not take
        self.mmax = self.nlon // 2 + 1
        self.mmax_local, self.mmax_offset = self.mmax, 0
        self.nlat_local, self.nlat_offset = self.nlat, 0
        nh = comm.get_size("h") if self.spatial_distributed else 1
        if self.spatial_distributed:
            if comm.get_size("w") > 1:
                raise NotImplementedError("ZonalSpectrumAverageBuffer with a split 'w' group needs a distributed planar FFT")
            shapes = thd.compute_split_shapes(self.nlat, nh)
            self.nlat_local = shapes[comm.get_rank("h")]
            self.nlat_offset = sum(shapes[:comm.get_rank("h")])
        self.lat_lon = lat_lon
        enssize = self._members(ensemble_size)
        super().__init__(num_rollout_steps=num_rollout_steps, rollout_dt=rollout_dt,
                         variable_shape=(enssize, self.nlat_local, self.mmax_local), channel_names=channel_names, device=device,
                         scale=scale, bias=bias, output_channels=output_channels, output_file=output_file)
        self.img_shape = img_shape
        self.bias = self.bias.reshape(1, 1, -1, 1, 1)
        self.scale = self.scale.reshape(1, 1, -1, 1, 1)
        lats = torch.tensor(self.lat_lon[0], dtype=torch.float32, device=self.device)
        w = torch.cos(torch.deg2rad(lats))                    # latitudes, hence the cosine
        if w.numel() != self.nlat:
            raise ValueError(f"lat_lon[0] has {w.numel()} latitudes for a grid of {self.nlat}")
        if nh > 1:
            w = thd.split_tensor_along_dim(w, dim=0, num_chunks=nh)[comm.get_rank("h")]
        self._latw = w.contiguous()
        self.lat_weights = torch.reshape(w, (1, 1, 1, -1, 1))

    @torch.no_grad()
    def update(self, data: torch.Tensor, targ: torch.Tensor, idt: int):
        self._check_step(idt)
        B, sources = self._sources(data, targ)
        C, E1 = self.num_channels, self.running_mean.shape[2]
        fw = 1.0 / self.nlon
        with torch.cuda.device(data.device):
            for x4, E, e0 in sources:
                if tuple(x4.shape[-2:]) != (self.nlat_local, self.nlon):
                    raise ValueError(f"expected (..., {self.nlat_local}, {self.nlon}), got {tuple(x4.shape)}")
                Cp = ops.round4(C)
                F = ops.rfft_rows(x4, self.mmax, Cp, (fw, fw, fw))                # (mmax, nlat_loc, 2, B * E * Cp)
                check(lib().mk_zonal_welford(ptr(F), ptr(self._scale), ptr(self._bias), ptr(self._latw), ptr(self.running_mean[idt]),
                                             ptr(self.running_var[idt]), ptr(self.num_samples_tracked[idt]),
                                             int(data.dtype == torch.bfloat16), self.mmax, self.nlat_local, F.shape[3], Cp, B, E, C, E1, e0,
                                             stream()), "mk_zonal_welford")
            self._advance(idt, B)
