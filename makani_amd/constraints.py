"""Physical output constraints between the network and the loss, on the HIP path (csrc/constraints.hip).

The interface of the reference: ``makani/utils/constraints.py`` (``NonNegativeConstraint``, ``HydrostaticBalanceProjection``,
``get_matching_channels_pl``) and ``makani/models/parametrizations.py`` (``_HydrostaticBalanceWrapper``, ``ConstraintsWrapper``):
constructor arguments, defaults, error types and messages, attributes and buffers (with their persistence, so that a reference
``state_dict`` loads with ``strict=True``).  The operators are built on the host in fp64 / fp32 exactly as the reference builds
them; ``forward`` is ONE launch that reads the prediction once and writes it once (``ops.ColumnMixFn`` / ``ops.NonNegFn``), in
fp32 whatever the dtype of ``x``, with the backward pass the transposed launch.  Two stated deviations: the non-negativity layer
is evaluated in fp32 and rounded once (the reference evaluates it in the dtype of ``x``), and channels-last or otherwise
non-contiguous inputs are made contiguous.  The layers are pointwise in space: a rank of an h x w split applies them to its
shard as it stands, nothing is exchanged.

``constrain_model_handle(params, model_handle, bias, scale)`` is the binding of ``params.constraints`` that
``makani/models/model_registry.py:179-187,240-255`` performs."""
import math
import re
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import device_guard, need_gpu

# makani/utils/constants.py
R_DRY_AIR = 287.052874247
Q_CORRECTION_MOIST_AIR = 0.6078

MAX_LEVELS = ops.CMIX_LEVELS


def get_matching_channels_pl(channel_names, prefix1, prefix2, p_min, p_max, revert=True):
    """the pressure levels two pressure-level variables share inside [p_min, p_max]: (indices of prefix1, of prefix2, levels)"""
    p1_pat = re.compile(r"^" + prefix1 + r"\d{1,}$")
    p2_pat = re.compile(r"^" + prefix2 + r"\d{1,}$")
    p1_pressures = [int(x.replace(prefix1, "")) for x in channel_names if p1_pat.match(x) is not None]
    p2_pressures = [int(x.replace(prefix2, "")) for x in channel_names if p2_pat.match(x) is not None]
    pressures = sorted([x for x in p1_pressures if ((x in p2_pressures) and (x >= p_min) and (x <= p_max))], reverse=revert)
    p1_idx = [channel_names.index(f"{prefix1}{p}") for p in pressures]
    p2_idx = [channel_names.index(f"{prefix2}{p}") for p in pressures]
    return p1_idx, p2_idx, pressures


def _check_levels(L):
    if L > MAX_LEVELS:
        raise ValueError(f"Error, {L} pressure levels: the HIP path keeps a column of at most {MAX_LEVELS} levels in registers.")


class _Tabled(nn.Module):
    """the device tables of a layer, rebuilt when a buffer they were made from changes (``load_state_dict``, ``.to``)"""

    _table_sources = ()

    def _table_key(self, device):
        return (device,) + tuple((b.data_ptr(), b._version) for b in (getattr(self, n, None) for n in self._table_sources) if b is not None)

    def _tables(self, device):
        key = self._table_key(device)
        if getattr(self, "_tab_key", None) != key:
            self._tab, self._tab_key = self._build_tables(device), key
        return self._tab


class NonNegativeConstraint(_Tabled):
    """Non-negativity of named channels in physical units (x_raw = scale x + bias >= 0): in training a soft clamp, "silu"
    ``w sigmoid(w / eps)`` or "softplus" ``leak w + (1 - leak) eps (softplus(w / eps) - ln 2)`` on ``w = x + bias / scale``; in
    evaluation the hard clamp.  Names not found are skipped; none found raises."""

    _table_sources = ("channel_indices", "offset")

    def __init__(self, channel_names, names_to_clamp, bias=None, scale=None, eps=0.1, mode="silu", leak=0.02):
        super().__init__()
        if mode not in ("silu", "softplus"):
            raise ValueError(f"NonNegativeConstraint mode must be 'silu' or 'softplus', got {mode!r}")
        self.eps = eps
        self.mode = mode
        self.leak = leak
        chan_idx = [channel_names.index(n) for n in names_to_clamp if n in channel_names]
        if not chan_idx:
            raise ValueError(f"None of the requested channel names {names_to_clamp} were found in channel_names.")
        self.num_channels = len(channel_names)
        self.register_buffer("channel_indices", torch.tensor(chan_idx, dtype=torch.long), persistent=False)
        if bias is not None and scale is not None:
            means = bias[0, chan_idx, 0, 0].to(torch.float32)
            stds = scale[0, chan_idx, 0, 0].to(torch.float32)
            self.register_buffer("offset", (means / stds).view(1, -1, 1, 1), persistent=False)
        else:
            self.offset = None

    def _build_tables(self, device):
        slot = torch.full((self.num_channels,), -1, dtype=torch.int32)
        slot[self.channel_indices.cpu()] = torch.arange(self.channel_indices.numel(), dtype=torch.int32)
        offset = None if self.offset is None else self.offset.detach().reshape(-1).to(device=device, dtype=torch.float32).contiguous()
        return slot.to(device), offset

    @device_guard
    def forward(self, x):
        need_gpu(x, "constraints")
        slot, offset = self._tables(x.device)
        mode = (0 if self.mode == "silu" else 1) if self.training else 2
        return ops.NonNegFn.apply(x, slot, offset, mode, float(self.eps), float(self.leak))


class HydrostaticBalanceProjection(_Tabled):
    """The minimum-norm (metric 1 / scale^2) projection of the predicted (T, Z) columns onto the hydrostatic balance manifold
    ``Z_i - Z_{i-1} = c_i (T_i + T_{i-1})``, ``c_i = R / 2 log(p_{i-1} / p_i)``:  ``x' = x - strength (P x - off)`` in physical
    units, with ``off`` from an optional ``climatology_offset`` (``A x = b_clim``) and, with ``use_moist_air_formula``, in (Tv, Z)
    with q held fixed."""

    _table_sources = ("channel_indices", "q_indices", "proj", "off", "scale_sub", "bias_sub", "q_scale", "q_bias")

    def __init__(self, channel_names, bias=None, scale=None, p_min=50, p_max=900, strength=1.0, use_moist_air_formula=False,
                 climatology_offset=None):
        super().__init__()
        self.strength = float(strength)
        self.use_moist_air_formula = use_moist_air_formula
        z_idx, t_idx, pressures = get_matching_channels_pl(channel_names, "z", "t", p_min, p_max)
        if len(pressures) < 2:
            raise ValueError("Error, need at least two overlapping z/t pressure levels to enforce hydrostatic balance.")
        L = len(pressures)
        _check_levels(L)
        self.num_channels = len(channel_names)
        all_idx = t_idx + z_idx
        self.register_buffer("channel_indices", torch.tensor(all_idx, dtype=torch.long), persistent=False)
        if self.use_moist_air_formula:
            q_idx, _, q_pressures = get_matching_channels_pl(channel_names, "q", "t", p_min, p_max)
            for p1, p2 in zip(pressures, q_pressures):
                if p1 != p2:
                    raise ValueError("Error, make sure that you have the same pressure levels for t, z and q channels")
            if len(q_idx) != L:
                raise ValueError("Error, make sure that you have the same pressure levels for t, z and q channels")
            self.q_prefact = Q_CORRECTION_MOIST_AIR
            self.register_buffer("q_indices", torch.as_tensor(q_idx, dtype=torch.long), persistent=False)

        # the constraint matrix A (L - 1, 2 L) on [T.., Z..] in physical units, fp64
        A = torch.zeros((L - 1, 2 * L), dtype=torch.float64)
        for i in range(1, L):
            c_i = 0.5 * R_DRY_AIR * math.log(pressures[i - 1] / pressures[i])
            r = i - 1
            A[r, L + i] = 1.0
            A[r, L + i - 1] = -1.0
            A[r, i] = -c_i
            A[r, i - 1] = -c_i

        def _gather(stat, idx, default):
            if stat is not None:
                return stat[0, idx, 0, 0].to(device="cpu", dtype=torch.float64)
            return torch.full((len(idx),), default, dtype=torch.float64)

        scale_sub = _gather(scale, all_idx, 1.0)
        bias_sub = _gather(bias, all_idx, 0.0)
        # x' = x - strength (P x - off),  P = M A,  off = M b_clim,  M = W^-1 A^T (A W^-1 A^T)^-1,  W = diag(1 / scale^2)
        Winv = scale_sub**2
        AWinv = A * Winv[None, :]
        M = (A.T * Winv[:, None]) @ torch.linalg.inv(AWinv @ A.T)
        Pphys = M @ A
        if climatology_offset is not None:
            b_clim_full = climatology_offset.to(device="cpu", dtype=torch.float64).reshape(-1)
            _, _, pressures_all = get_matching_channels_pl(channel_names, "z", "t", float("-inf"), float("inf"))
            if b_clim_full.shape[0] != len(pressures_all) - 1:
                raise ValueError(
                    f"climatology_offset must have length {len(pressures_all) - 1} (one per interior level "
                    f"over all {len(pressures_all)} matching z/t pressure levels), got {b_clim_full.shape[0]}."
                )
            start = pressures_all.index(pressures[0])
            off = M @ b_clim_full[start: start + (L - 1)]
        else:
            off = torch.zeros(2 * L, dtype=torch.float64)

        self.register_buffer("proj", Pphys.float(), persistent=False)
        self.register_buffer("off", off.float().view(1, -1, 1, 1), persistent=False)
        self.register_buffer("scale_sub", scale_sub.float().view(1, -1, 1, 1), persistent=False)
        self.register_buffer("bias_sub", bias_sub.float().view(1, -1, 1, 1), persistent=False)
        if self.use_moist_air_formula:
            self.register_buffer("q_scale", _gather(scale, q_idx, 1.0).float().view(1, -1, 1, 1), persistent=False)
            self.register_buffer("q_bias", _gather(bias, q_idx, 0.0).float().view(1, -1, 1, 1), persistent=False)
        self.num_levels = L

    def _build_tables(self, device):
        L, C = self.num_levels, self.num_channels
        rows = self.channel_indices.tolist()
        q = self.q_indices.tolist() if self.use_moist_air_formula else []
        rest = [c for c in range(C) if c not in rows and c not in q]
        n_m = L if q else 0
        return ops.column_mix(rows, rows, q, q, rest, rest, self.scale_sub, self.bias_sub, self.scale_sub, self.bias_sub, self.off,
                              self.q_scale if q else None, self.q_bias if q else None, self.proj, C, C, n_m, n_m, True, False,
                              -self.strength, self.q_prefact if q else 0.0, device)

    @device_guard
    def forward(self, x):
        need_gpu(x, "constraints")
        return ops.ColumnMixFn.apply(x, self._tables(x.device))


class _HydrostaticBalanceWrapper(_Tabled):
    """The full temperature column from one reference temperature and the geopotentials: the input carries ``C - L + 1``
    channels ``[T_0, Z_0 .. Z_{L-1}, (q_0 .. q_{L-1},) the rest]``, the output the ``C`` named ones, with
    ``T_i = 2 (Z_i - Z_{i-1}) / (R log(p_{i-1} / p_i)) - T_{i-1}`` in physical units (virtual temperature with
    ``use_moist_air_formula``)."""

    _table_sources = ("mapping", "inp_scale", "inp_bias", "out_scale", "out_bias")

    def __init__(self, channel_names, bias, scale, p_min=50, p_max=900, use_moist_air_formula=False):
        super().__init__()
        self.use_moist_air_formula = use_moist_air_formula
        self.z_idx, self.t_idx, self.pressures = get_matching_channels_pl(channel_names, "z", "t", p_min, p_max)
        if self.use_moist_air_formula:
            self.q_idx, _, p_tmp = get_matching_channels_pl(channel_names, "q", "t", p_min, p_max)
        if len(self.pressures) == 0:
            raise ValueError("Error, make sure that you have overlapping pressure levels for geopotential and temperature")
        if self.use_moist_air_formula:
            for p1, p2 in zip(self.pressures, p_tmp):
                if p1 != p2:
                    raise ValueError("Error, make sure that you have the same pressure levels for t,z and q channels")
            if len(self.q_idx) != len(self.pressures):
                raise ValueError("Error, make sure that you have the same pressure levels for t,z and q channels")
        L = len(self.pressures)
        _check_levels(L)
        self.num_levels = L

        self.aux_idx = [i for i in range(len(channel_names)) if (i not in self.t_idx + self.z_idx)]
        if self.use_moist_air_formula:
            self.aux_idx = [i for i in self.aux_idx if (i not in self.q_idx)]
        self.prefact = 1.0 / R_DRY_AIR
        if self.use_moist_air_formula:
            self.q_prefact = Q_CORRECTION_MOIST_AIR
        nq = len(self.q_idx) if self.use_moist_air_formula else 0

        def stat(t, idx, default):
            if t is not None:
                return t[:, idx, ...]
            return torch.full([1, len(idx), 1, 1], default, dtype=torch.float32)

        z_bias, t_bias = stat(bias, self.z_idx, 0.0), stat(bias, self.t_idx, 0.0)
        z_scale, t_scale = stat(scale, self.z_idx, 1.0), stat(scale, self.t_idx, 1.0)
        if self.use_moist_air_formula:
            q_bias, q_scale = stat(bias, self.q_idx, 0.0), stat(scale, self.q_idx, 1.0)

        # the (C, C - L + 1) map of the reference, entry by entry in its order (equal indices are summed, as `coalesce` does)
        row_indices, col_indices, values = [self.t_idx[0]], [0], [1.0]
        for idx in range(1, L + 1):
            row_indices.append(self.z_idx[idx - 1])
            col_indices.append(idx)
            values.append(1.0)
        for oidx in range(1, L):
            for iidx in range(0, oidx):
                sign = (-1.0) ** (oidx + iidx - 1)
                plog = np.log(self.pressures[iidx] / self.pressures[iidx + 1])
                row_indices += [self.t_idx[oidx], self.t_idx[oidx]]
                col_indices += [iidx + 2, iidx + 1]
                values += [sign * 2.0 * self.prefact / plog, -sign * 2.0 * self.prefact / plog]
            row_indices.append(self.t_idx[oidx])
            col_indices.append(0)
            values.append((-1.0) ** oidx)
        off_idx = L + 1
        for j in range(nq):
            row_indices.append(self.q_idx[j])
            col_indices.append(off_idx + j)
            values.append(1.0)
        off_idx += nq
        for j, a in enumerate(self.aux_idx):
            row_indices.append(a)
            col_indices.append(off_idx + j)
            values.append(1.0)
        ncols = len(channel_names) - len(self.t_idx) + 1
        indices = torch.tensor([row_indices, col_indices], dtype=torch.long)
        values = torch.tensor(values, dtype=torch.float32)
        mapping = torch.sparse_coo_tensor(indices, values, size=(len(channel_names), ncols)).coalesce().to_dense()
        self.register_buffer("mapping", mapping, persistent=False)

        inp_scale = torch.ones((1, ncols, 1, 1), dtype=torch.float32)
        inp_scale[0, 0, 0, 0] = t_scale[0, 0, 0, 0]
        inp_scale[0, 1: L + 1, 0, 0] = z_scale[0, :, 0, 0]
        inp_bias = torch.zeros((1, ncols, 1, 1), dtype=torch.float32)
        inp_bias[0, 0, 0, 0] = t_bias[0, 0, 0, 0]
        inp_bias[0, 1: L + 1, 0, 0] = z_bias[0, :, 0, 0]
        if self.use_moist_air_formula:
            inp_bias[0, L + 1: L + nq + 1, 0, 0] = q_bias[0, :, 0, 0]
            inp_scale[0, L + 1: L + nq + 1, 0, 0] = q_scale[0, :, 0, 0]
        self.register_buffer("inp_scale", inp_scale, persistent=True)
        self.register_buffer("inp_bias", inp_bias, persistent=True)

        out_scale = torch.ones((1, len(channel_names), 1, 1), dtype=torch.float32)
        out_scale[:, self.t_idx, ...] = t_scale[...].to(torch.float32)
        out_scale[:, self.z_idx, ...] = z_scale[...].to(torch.float32)
        out_bias = torch.zeros((1, len(channel_names), 1, 1), dtype=torch.float32)
        out_bias[:, self.t_idx, ...] = t_bias[...].to(torch.float32)
        out_bias[:, self.z_idx, ...] = z_bias[...].to(torch.float32)
        if self.use_moist_air_formula:
            out_bias[:, self.q_idx, ...] = q_bias[...].to(torch.float32)
            out_scale[:, self.q_idx, ...] = q_scale[...].to(torch.float32)
        self.register_buffer("out_scale", out_scale, persistent=True)
        self.register_buffer("out_bias", out_bias, persistent=True)

    def _build_tables(self, device):
        L, C = self.num_levels, self.mapping.shape[0]
        nq = len(self.q_idx) if self.use_moist_air_formula else 0
        rows_out = self.t_idx + self.z_idx
        rows_in = list(range(L + 1))
        q_in = list(range(L + 1, L + 1 + nq))
        q_out = self.q_idx if nq else []
        copy_src = list(range(L + 1 + nq, self.mapping.shape[1]))
        isc, ibi = self.inp_scale.reshape(-1), self.inp_bias.reshape(-1)
        osc, obi = self.out_scale.reshape(-1), self.out_bias.reshape(-1)
        return ops.column_mix(rows_in, rows_out, q_in, q_out, copy_src, self.aux_idx, isc[: L + 1], ibi[: L + 1], osc[rows_out], obi[rows_out],
                              None, isc[L + 1: L + 1 + nq] if nq else None, ibi[L + 1: L + 1 + nq] if nq else None,
                              self.mapping[rows_out][:, : L + 1], self.mapping.shape[1], C, 1 if nq else 0, L if nq else 0, False, True,
                              1.0, self.q_prefact if nq else 0.0, device)

    @device_guard
    def forward(self, inp: torch.Tensor) -> torch.Tensor:
        need_gpu(inp, "constraints")
        return ops.ColumnMixFn.apply(inp, self._tables(inp.device))


class ConstraintsWrapper(nn.Module):
    """A model (``model_handle``, a zero-argument factory) followed by the first configured constraint, or the constraint alone.
    ``constraints`` is a list of ``{"type": "hydrostatic_balance", "options": {...}}``; ``N_in_channels`` is the number of
    channels the wrapped model has to produce."""

    def __init__(self, constraints, channel_names, bias, scale, model_handle=None):
        super().__init__()
        self.model = model_handle() if model_handle is not None else None
        self.constraint_list = nn.ModuleList()
        for constraint in constraints:
            if constraint["type"] == "hydrostatic_balance":
                self.constraint_list.append(
                    _HydrostaticBalanceWrapper(**constraint["options"], channel_names=channel_names, bias=bias, scale=scale)
                )
                self.N_in_channels = self.constraint_list[-1].mapping.shape[1]
            else:
                raise NotImplementedError("Error, constraints different from hydrostatic balance are not yet implemented.")

    def forward(self, inp: torch.Tensor) -> torch.Tensor:
        if self.model is not None:
            inp = self.model(inp)
        # the reference applies the first constraint only
        return self.constraint_list[0](inp)


def constrain_model_handle(params, model_handle, bias, scale):
    """``(wrapped_handle, out_chans)`` for a recipe with ``params.constraints`` (makani/models/model_registry.py:179-187,240-255):
    ``model_handle`` is a factory that still takes ``out_chans=``; the wrapped handle builds ``ConstraintsWrapper`` around it with
    ``out_chans`` reduced to the wrapper's ``N_in_channels``.  ``bias`` / ``scale`` are the (1, C, 1, 1) statistics of the output
    channels (reading the stats files is the host's job).  Without ``params.constraints`` the handle comes back as it is, with
    ``out_chans = params.N_out_channels``."""
    get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
    constraints = get("constraints", None)
    if constraints is None:
        return model_handle, get("N_out_channels", None)
    names = get("channel_names", None)
    out_chans = ConstraintsWrapper(constraints=constraints, channel_names=names, bias=None, scale=None, model_handle=None).N_in_channels
    if bias is not None:
        bias = torch.as_tensor(bias).to(torch.float32)
    if scale is not None:
        scale = torch.as_tensor(scale).to(torch.float32)
    # (a keyword given here replaces an `out_chans` the handle had bound already)
    wrapped = partial(ConstraintsWrapper, constraints=constraints, channel_names=names, bias=bias, scale=scale,
                      model_handle=partial(model_handle, out_chans=out_chans))
    return wrapped, out_chans
