"""Imputation of missing input values on the HIP path (csrc/impute.hip).

The interface of the reference, ``makani/models/common/imputation.py``: constructor arguments (spelling included), attributes,
``state_dict`` keys and shapes, the ``is_shared_mp`` annotations, any number of leading batch dimensions and ``mask=None``.
``forward`` is ONE launch that reads ``x`` once and writes the result once (``ops.ImputeMlpFn`` / ``ops.ImputeConstFn``), in fp32
whatever the dtype of ``x``; the backward pass recomputes the hidden layer from the saved input and mask.

``MLPImputation`` takes one more, keyword-only argument: ``mask_channel=c`` reads the mask from channel ``c`` of ``x`` itself (any
nonzero value counts), the form a network uses whose land mask travels among its input channels; no slice is copied.

Stated deviations: under autocast the MLP still runs in fp32 (the reference rounds its convolutions to the autocast dtype);
non-contiguous inputs are made contiguous; the MLP holds at most ``ops.IMPUTE_CHANNELS`` input channels, ``ops.IMPUTE_SLOTS``
imputed channels and ``ops.IMPUTE_HIDDEN`` hidden units (more raise ``NotImplementedError``), its activation is GELU, ReLU, SiLU
or sin.  The layers are pointwise in space: a rank of an h x w split applies them to its shard as it stands."""
from typing import Optional

import torch
import torch.nn as nn

from . import comm, ops
from ._lib import device_guard, need_gpu
from .layers import EncoderDecoder


class Sin(nn.Module):
    """the ``sin`` activation of FourCastNet3.1"""

    def forward(self, x):
        return torch.sin(x)


def activation_code(activation_function) -> int:
    """the code of ``mk_impute_mlp_fwd`` for an activation class (or instance) of the four the kernel evaluates"""
    cls = activation_function if isinstance(activation_function, type) else type(activation_function)
    if cls is nn.GELU:
        if not isinstance(activation_function, type) and getattr(activation_function, "approximate", "none") != "none":
            raise NotImplementedError("MLPImputation on the HIP path evaluates the exact (erf) GELU, not the tanh approximation")
        return ops.IMPUTE_ACTS["gelu"]
    for name, c in (("relu", nn.ReLU), ("silu", nn.SiLU), ("sin", Sin)):
        if cls is c:
            return ops.IMPUTE_ACTS[name]
    if cls.__name__ == "Sin" and cls.__module__ == "makani.models.networks.fourcastnet3_1":          # the reference's own wrapper of torch.sin
        return ops.IMPUTE_ACTS["sin"]
    raise NotImplementedError(f"MLPImputation on the HIP path evaluates GELU, ReLU, SiLU or Sin, not {cls.__name__}")


class MLPImputation(nn.Module):
    """Masked entries (NaN, or flagged by ``mask``) of the channels ``inpute_chans`` are replaced by the prediction of a one-layer MLP
    over all ``inp_chans`` channels, whose input has zeros there; everything else passes through bit for bit."""

    def __init__(self, inp_chans: int = 2, inpute_chans: torch.Tensor = torch.tensor([0]), mlp_ratio: float = 2.0,
                 activation_function: nn.Module = nn.GELU, *, mask_channel: Optional[int] = None):
        super().__init__()
        self.inp_chans = inp_chans
        self.inpute_chans = inpute_chans
        self.out_chans = inpute_chans.shape[0]
        self.mask_channel = mask_channel
        hidden = int(mlp_ratio * self.out_chans)
        self.act_code = activation_code(activation_function)
        ops.impute_check(inp_chans, self.out_chans, hidden)
        if mask_channel is not None and not 0 <= mask_channel < inp_chans:
            raise ValueError(f"mask channel {mask_channel} outside the {inp_chans} input channels")
        self.mlp = EncoderDecoder(num_layers=1, input_dim=inp_chans, output_dim=self.out_chans, hidden_dim=hidden,
                                  act_layer=activation_function, input_format="nchw")
        self._itab = {}
        self._tab, self._tab_key = None, None

    def _table(self, device):
        if device not in self._itab:
            self._itab[device] = ops.impute_itab(self.inpute_chans.tolist(), self.inp_chans, device)
        return self._itab[device]

    def _weights(self):
        fc1, fc2 = self.mlp.fwd[0], self.mlp.fwd[2]
        hidden = fc1.weight.shape[0]
        return fc1.weight.view(hidden, self.inp_chans), fc1.bias, fc2.weight.view(self.out_chans, hidden)

    def _weight_table(self, device):
        """the device table of the kernels: rebuilt (a handful of small launches) only when a parameter has changed"""
        ps = (self.mlp.fwd[0].weight, self.mlp.fwd[0].bias, self.mlp.fwd[2].weight)
        key = (device,) + tuple((p.data_ptr(), p._version) for p in ps)
        if self._tab_key != key or torch.cuda.is_current_stream_capturing():
            w1, b1, w2 = self._weights()
            tab = ops.impute_table(w1.float(), b1.float(), w2.float(), self._table(device))
            if torch.cuda.is_current_stream_capturing():          # a replay must read the weights of its own time
                return tab
            self._tab, self._tab_key = tab, key
        return self._tab

    def impute(self, x, mask=None, mask_channel=None):
        need_gpu(x, "imputation")
        with torch.autocast(device_type="cuda", enabled=False):
            return ops.ImputeMlpFn.apply(x, *self._weights(), self._weight_table(x.device), mask, mask_channel, self.act_code)

    @device_guard
    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None):
        return self.impute(x, mask, self.mask_channel)


class ConstantImputation(nn.Module):
    """Masked entries (NaN, or flagged by a ``mask`` broadcastable to ``x``) are replaced by one learned constant per channel."""

    def __init__(self, inp_chans: int = 2):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(inp_chans, 1, 1))
        if comm.get_size("spatial") > 1:
            self.weight.is_shared_mp = ["spatial"]
            self.weight.sharded_dims_mp = [None, None, None]

    @device_guard
    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None):
        need_gpu(x, "imputation")
        with torch.autocast(device_type="cuda", enabled=False):
            return ops.ImputeConstFn.apply(x, self.weight, mask)
