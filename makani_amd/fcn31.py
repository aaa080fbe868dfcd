"""FourCastNet3.1 (``AtmoSphericNeuralOperatorNet31``, ``makani/models/networks/fourcastnet3_1.py``, ``nettype: "FCN3.1"``) on the
MI355X HIP path.

Same constructor keywords (unknown ones are accepted and ignored), construction order (it is the RNG stream of the
initialisation), ``state_dict`` keys and shapes, non-persistent index buffers (history offsets included) and methods
(``impute_sst_channels``, ``encode``, ``encode_auxiliary_channels``, ``decode``, ``processor_blocks``, ``clamp_water_channels``,
``forward``) as the reference.  What differs from FourCastNet3 (``fcn3.py``): ONE DISCO encoder / decoder pair over all prognostic
channels; the cutoff radius ``margin kernel_shape[0] pi / lmax`` with no doubling in the blocks; a triangular ``lmax = mmax``
transform pair from ``compute_spherical_bandlimit``; block gain 0.5, ``SpectralConv(bias=False)``, and a convolution that changes
the channel count when ``use_mlp=False``; a ``LearnablePositionEmbedding`` among the auxiliary embeddings; history; the ``sin``
activation; an identity big skip on ``pred_channels``; learned imputation of NaN sea-surface temperature.

The two stages at the full data grid are one launch per direction each (``csrc/impute.hip``): ``forward`` imputes with the land mask
read from the ``xlsml`` channel of ``x`` itself (``MLPImputation(mask_channel=)``) and ends in ``ops.Fcn31TailFn`` (skip + water
clamp).  ``impute_sst_channels`` and ``clamp_water_channels`` as public methods keep the reference's composed form.  The output
stays in ``surf + atmo`` order and the clamp indexes it with ``water_channels`` as the reference does (``fourcastnet3_1.py:1068``).

Stated deviations: ``fused=`` is accepted and ignored; ``basis_type`` "harmonic" / "fourier-bessel" and ``basis_norm_mode="nodal"``
raise ``NotImplementedError`` (in no torch-harmonics release whose source is known here, see ``oracle/disco.py``; the sub-classes
keep the reference's default signatures); the position embedding is expanded over the batch, so B > 1 works where the reference's
``cat`` raises; under bf16 autocast the imputation MLP runs in fp32; non-contiguous inputs are made contiguous; the imputation's
capacities (``makani_amd/imputation.py``).
"""
import math

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from . import ops
from ._lib import device_guard
from . import distributed as thd
from .disco import DistributedResampleS2, ResampleS2
from .fcn3 import (LayerScale, _annotate_spatial, _conv_handle, _norm_handle, _soft_clamp, _spatial_parallel, get_channel_groups,
                   get_water_channels)
from .imputation import MLPImputation, Sin
from .layers import MLP, DropPath, PointwiseConv
from .sht import InverseRealSHT, RealSHT
from .spectral_conv import SpectralConv


# makani/utils/grids.py:43-54
def compute_spherical_bandlimit(img_shape, grid_type):
    if grid_type == "equiangular":
        return min((img_shape[0] - 1) // 2, img_shape[1] // 2)
    if grid_type == "legendre-gauss":
        return min(img_shape[0] - 1, img_shape[1] // 2)
    raise NotImplementedError(f"Unknown type {grid_type} not implemented")


# fourcastnet3_1.py:55-57
def _compute_cutoff_radius(lmax, kernel_shape, basis_type):
    margin_factor = {"piecewise linear": 1.0, "morlet": 1.0, "harmonic": 1.0, "zernike": 1.0, "fourier-bessel": 1.5}
    return margin_factor[basis_type] * kernel_shape[0] * math.pi / float(lmax)


def _check_basis(basis_type, basis_norm_mode):
    if basis_type in ("harmonic", "fourier-bessel"):
        raise NotImplementedError(f"filter basis {basis_type!r} is in no torch-harmonics release whose source is known here; "
                                  "built are 'morlet', 'piecewise linear' and 'zernike'")
    if basis_norm_mode == "nodal":
        raise NotImplementedError("basis_norm_mode='nodal' is in no torch-harmonics release whose source is known here; "
                                  "built are 'none', 'individual', 'mean' and 'support'")


def _disco(inp_chans, out_chans, in_shape, out_shape, kernel_shape, basis_type, basis_norm_mode, grid_in, grid_out, groups, bias, lmax):
    _check_basis(basis_type, basis_norm_mode)
    conv = _conv_handle()(inp_chans, out_chans, in_shape=in_shape, out_shape=out_shape, kernel_shape=kernel_shape,
                          basis_type=basis_type, basis_norm_mode=basis_norm_mode, grid_in=grid_in, grid_out=grid_out, groups=groups,
                          bias=bias, theta_cutoff=_compute_cutoff_radius(lmax=lmax, kernel_shape=kernel_shape, basis_type=basis_type))
    if _spatial_parallel():
        _annotate_spatial(conv)
    return conv


# makani/models/common/pos_embedding.py:67-151
class LearnablePositionEmbedding(nn.Module):
    """learned position embedding, per latitude ring ("lat") or per grid point ("latlon"), at the rank's LOCAL shape"""

    def __init__(self, img_shape=(480, 960), grid="equiangular", num_chans=1, embed_type="lat"):
        super().__init__()
        self.img_shape, self.num_chans = img_shape, num_chans
        par = _spatial_parallel()          # (the transform layer's groups: set by hand or taken from the process-group tree)
        nh, nw = (thd.polar_group_size(), thd.azimuth_group_size()) if par else (1, 1)
        self.local_shape_h = thd.compute_split_shapes(img_shape[0], nh)[thd.polar_group_rank()] if nh > 1 else img_shape[0]
        self.local_shape_w = thd.compute_split_shapes(img_shape[1], nw)[thd.azimuth_group_rank()] if nw > 1 else img_shape[1]
        if embed_type == "latlon":
            self.position_embeddings = nn.Parameter(torch.zeros(1, num_chans, self.local_shape_h, self.local_shape_w))
            self.position_embeddings.is_shared_mp = []
            self.position_embeddings.sharded_dims_mp = [None, None, "h", "w"]
        elif embed_type == "lat":
            self.position_embeddings = nn.Parameter(torch.zeros(1, num_chans, self.local_shape_h, 1))
            self.position_embeddings.is_shared_mp = ["w"]
            self.position_embeddings.sharded_dims_mp = [None, None, "h", None]
        else:
            raise ValueError(f"Unknown learnable position embedding type {embed_type}")

    def forward(self):
        return self.position_embeddings.expand(-1, -1, self.local_shape_h, self.local_shape_w)


class DiscreteContinuousEncoder(nn.Module):
    def __init__(self, inp_shape=(721, 1440), out_shape=(480, 960), grid_in="equiangular", grid_out="equiangular", inp_chans=2,
                 out_chans=2, kernel_shape=(3, 3), basis_type="harmonic", basis_norm_mode="nodal", lmax=240, groups=1, bias=False,
                 fused=False):
        super().__init__()
        self.conv = _disco(inp_chans, out_chans, inp_shape, out_shape, kernel_shape, basis_type, basis_norm_mode, grid_in, grid_out,
                           groups, bias, lmax)

    def forward(self, x):
        return self.conv(x)


class DiscreteContinuousDecoder(nn.Module):
    def __init__(self, inp_shape=(480, 960), out_shape=(721, 1440), grid_in="equiangular", grid_out="equiangular", inp_chans=2,
                 out_chans=2, kernel_shape=(3, 3), basis_type="harmonic", basis_norm_mode="nodal", lmax=240, resample_sht=False,
                 groups=1, bias=False, fused=False):
        super().__init__()
        _check_basis(basis_type, basis_norm_mode)
        par = _spatial_parallel()
        if resample_sht:
            sht, isht = (thd.DistributedRealSHT, thd.DistributedInverseRealSHT) if par else (RealSHT, InverseRealSHT)
            self.sht = sht(*inp_shape, grid=grid_in).float()
            self.isht = isht(*out_shape, lmax=self.sht.lmax, mmax=self.sht.mmax, grid=grid_out).float()
            self.resample = nn.Sequential(self.sht, self.isht)
        else:
            self.resample = (DistributedResampleS2 if par else ResampleS2)(*inp_shape, *out_shape, grid_in=grid_in,
                                                                            grid_out=grid_out, mode="bilinear")
        self.conv = _disco(inp_chans, out_chans, out_shape, out_shape, kernel_shape, basis_type, basis_norm_mode, grid_out, grid_out,
                           groups, bias, lmax)

    def forward(self, x):
        dtype = x.dtype
        with torch.autocast(device_type=x.device.type, enabled=False):      # the reference resamples in fp32 ...
            res = self.resample(x.float()).to(dtype=dtype)
        return self.conv(res)                                               # ... and convolves in the caller's dtype


class NeuralOperatorBlock(nn.Module):
    """norm1 -> global (spectral) or local (DISCO) convolution -> norm2 -> MLP -> skip(x[:out_chans]) + layer_scale(dx); without the
    MLP the convolution itself maps inp_chans -> out_chans"""

    def __init__(self, forward_transform, inverse_transform, inp_chans, out_chans, conv_type="local", mlp_ratio=2.0,
                 mlp_drop_rate=0.0, path_drop_rate=0.0, act_layer=nn.GELU, normalization_layer="none", num_groups=1,
                 skip="identity", layer_scale=True, use_mlp=False, kernel_shape=(3, 3), basis_type="harmonic",
                 basis_norm_mode="nodal", lmax=240, checkpointing_level=0, bias=False, fused=False):
        super().__init__()
        self.inp_shape = (forward_transform.nlat, forward_transform.nlon)
        self.out_shape = (inverse_transform.nlat, inverse_transform.nlon)
        self.out_chans = out_chans
        gain_factor = 0.5
        conv_out = inp_chans if use_mlp else out_chans
        if conv_type == "local":
            self.local_conv = _disco(inp_chans, conv_out, self.inp_shape, self.out_shape, kernel_shape, basis_type, basis_norm_mode,
                                     forward_transform.grid, inverse_transform.grid, num_groups, False, lmax)
            with torch.no_grad():
                self.local_conv.weight *= gain_factor
        elif conv_type == "global":
            self.global_conv = SpectralConv(forward_transform, inverse_transform, inp_chans, conv_out, operator_type="dhconv",
                                            num_groups=num_groups, bias=False, gain=gain_factor)
        else:
            raise ValueError(f"Unknown convolution type {conv_type}")
        handle = _norm_handle(self.inp_shape[0], self.inp_shape[1], inp_chans, normalization_layer=normalization_layer,
                              sht_grid_type=forward_transform.grid)
        self.norm1 = handle()
        self.norm2 = handle()
        if use_mlp:
            self.mlp = MLP(in_features=inp_chans, out_features=out_chans, hidden_features=int(inp_chans * mlp_ratio),
                           act_layer=act_layer, drop_rate=mlp_drop_rate, drop_type="features",
                           checkpointing=(checkpointing_level >= 2), gain=gain_factor)
        self.drop_path = DropPath(path_drop_rate) if path_drop_rate > 0.0 else nn.Identity()
        if layer_scale:
            self.layer_scale = LayerScale(out_chans)
            self.layer_scale.weight.is_shared_mp = ["spatial"]
            self.layer_scale.weight.sharded_dims_mp = [None, None, None, None]
        else:
            self.layer_scale = nn.Identity()
        if skip == "linear":
            self.skip = PointwiseConv(inp_chans, out_chans, bias=False)
            nn.init.normal_(self.skip.weight, std=math.sqrt(1.0 / inp_chans))
            self.skip.weight.is_shared_mp = ["spatial"]
            self.skip.weight.sharded_dims_mp = [None, None, None, None]
        elif skip == "identity":
            self.skip = nn.Identity()
        elif skip != "none":
            raise ValueError(f"Unknown skip connection type {skip}")

    def forward(self, x):
        x = self.norm1(x)
        if hasattr(self, "global_conv"):
            dx, _ = self.global_conv(x)
        else:
            dx = self.local_conv(x)
        dx = self.norm2(dx)
        if hasattr(self, "mlp"):
            dx = self.mlp(dx)
        dx = self.drop_path(dx)
        if hasattr(self, "skip"):
            res = self.skip(x[..., : self.out_chans, :, :])
            if isinstance(self.layer_scale, LayerScale):                          # skip + w[c] * dx in one pass
                return torch.addcmul(res, dx, self.layer_scale.weight.view(1, -1, 1, 1).to(dx.dtype))
            return res + self.layer_scale(dx)
        return dx


class AtmoSphericNeuralOperatorNet31(nn.Module):
    def __init__(self, model_grid_type="equiangular", sht_grid_type="legendre-gauss", inp_shape=(721, 1440), out_shape=(721, 1440),
                 kernel_shape=(3, 3), filter_basis_type="harmonic", filter_basis_norm_mode="mean", resample_sht=False,
                 channel_names=("u500", "v500"), aux_channel_names=(), n_history=0, embed_dim=8, aux_embed_dim=8, pos_embed_dim=0,
                 num_layers=4, num_groups=1, use_mlp=True, mlp_ratio=2.0, activation_function="gelu", layer_scale=True,
                 pos_drop_rate=0.0, path_drop_rate=0.0, mlp_drop_rate=0.0, normalization_layer="none",
                 hard_thresholding_fraction=0.25, scale_factor=8, lmax=None, sfno_block_frequency=2, big_skip=False,
                 clamp_water=False, encoder_bias=False, bias=False, checkpointing_level=0, freeze_encoder=False,
                 freeze_processor=False, normalization_means=None, normalization_stds=None, fused=True, **kwargs):
        super().__init__()
        self.inp_shape, self.out_shape = tuple(inp_shape), tuple(out_shape)
        self.embed_dim, self.aux_embed_dim, self.pos_embed_dim = embed_dim, aux_embed_dim, pos_embed_dim
        self.big_skip = big_skip
        self.checkpointing_level = checkpointing_level
        self.n_history = n_history
        self.h = int(self.inp_shape[0] // scale_factor)
        self.w = int(self.inp_shape[1] // scale_factor)
        if normalization_means is not None:
            self.register_buffer("normalization_means", torch.as_tensor(normalization_means))
        if normalization_stds is not None:
            self.register_buffer("normalization_stds", torch.as_tensor(normalization_stds))
        channel_names, aux_channel_names = list(channel_names), list(aux_channel_names)
        self._init_spectral_transforms(model_grid_type, sht_grid_type, hard_thresholding_fraction, lmax)
        self._precompute_channel_groups(channel_names, aux_channel_names, n_history)
        self.n_out_chans = self.n_atmo_groups * self.n_atmo_chans + self.n_surf_chans
        self.n_in_chans = self.n_out_chans * (self.n_history + 1)
        self.total_aux_embed_dim = (self.aux_embed_dim if self.n_aux_chans > 0 else 0) + self.pos_embed_dim
        kernel_shape = tuple(kernel_shape)
        try:
            act = {"relu": nn.ReLU, "gelu": nn.GELU, "silu": nn.SiLU, "sin": Sin}[activation_function]
        except KeyError:
            raise ValueError(f"Unknown activation function {activation_function}")

        # construction order = the reference's (it is the RNG stream of the initialisation)
        if self.sst_channels_in.shape[0] > 0:
            lsm = self.land_mask_channels.tolist()
            self.sst_imputation = MLPImputation(inp_chans=self.n_in_chans + self.n_aux_chans, inpute_chans=self.sst_channels_in,
                                                mlp_ratio=mlp_ratio, activation_function=act, mask_channel=lsm[0] if lsm else None)
        common = dict(kernel_shape=kernel_shape, basis_type=filter_basis_type, basis_norm_mode=filter_basis_norm_mode, lmax=self.lmax,
                      bias=encoder_bias, fused=fused)
        self.encoder = DiscreteContinuousEncoder(inp_shape=self.inp_shape, out_shape=(self.h, self.w), inp_chans=self.n_in_chans,
                                                 out_chans=embed_dim, grid_in=model_grid_type, grid_out=sht_grid_type,
                                                 groups=math.gcd(self.n_in_chans, embed_dim), **common)
        if self.n_aux_chans > 0:
            self.aux_encoder = DiscreteContinuousEncoder(inp_shape=self.inp_shape, out_shape=(self.h, self.w), inp_chans=self.n_aux_chans,
                                                         out_chans=aux_embed_dim, grid_in=model_grid_type, grid_out=sht_grid_type,
                                                         groups=math.gcd(self.n_aux_chans, aux_embed_dim), **common)
        self.decoder = DiscreteContinuousDecoder(inp_shape=(self.h, self.w), out_shape=self.out_shape, inp_chans=embed_dim,
                                                 out_chans=self.n_out_chans, grid_in=sht_grid_type, grid_out=model_grid_type,
                                                 groups=math.gcd(self.n_out_chans, embed_dim), resample_sht=resample_sht, **common)
        if self.pos_embed_dim > 0:
            self.pos_embed = LearnablePositionEmbedding(img_shape=(self.h, self.w), grid=sht_grid_type, num_chans=self.pos_embed_dim,
                                                        embed_type="lat")
        self.pos_drop = nn.Dropout(p=pos_drop_rate) if pos_drop_rate > 0.0 else nn.Identity()
        dpr = [v.item() for v in torch.linspace(0, path_drop_rate, num_layers)]
        self.blocks = nn.ModuleList([])
        for i in range(num_layers):
            conv_type = "global" if (sfno_block_frequency > 0 and i % sfno_block_frequency == 0) else "local"
            self.blocks.append(NeuralOperatorBlock(
                self.sht, self.isht, embed_dim + self.total_aux_embed_dim, embed_dim, conv_type=conv_type, mlp_ratio=mlp_ratio,
                mlp_drop_rate=mlp_drop_rate, path_drop_rate=dpr[i], act_layer=act, normalization_layer=normalization_layer,
                skip="identity", layer_scale=layer_scale, use_mlp=use_mlp, kernel_shape=kernel_shape, basis_type=filter_basis_type,
                basis_norm_mode=filter_basis_norm_mode, lmax=self.lmax, checkpointing_level=checkpointing_level, bias=bias, fused=fused))
        if clamp_water:
            water = get_water_channels(channel_names)
            if len(water) > 0:
                self.register_buffer("water_channels", torch.tensor(water, dtype=torch.long), persistent=False)
        if freeze_encoder:
            frozen = list(self.encoder.parameters()) + list(self.decoder.parameters())
            if hasattr(self, "aux_encoder"):
                frozen += list(self.aux_encoder.parameters())
            for p in frozen:
                p.requires_grad = False
        if freeze_processor:
            for p in self.blocks.parameters():
                p.requires_grad = False
        self._tail = {}

    def _init_spectral_transforms(self, model_grid_type="equiangular", sht_grid_type="legendre-gauss", hard_thresholding_fraction=1.0,
                                  lmax=None):
        if lmax is None:
            lmax = int(compute_spherical_bandlimit(self.inp_shape, model_grid_type) * hard_thresholding_fraction)
        self.lmax = lmax
        sht, isht = (thd.DistributedRealSHT, thd.DistributedInverseRealSHT) if _spatial_parallel() else (RealSHT, InverseRealSHT)
        self.sht = sht(self.h, self.w, lmax=self.lmax, mmax=self.lmax, grid=sht_grid_type).float()
        self.isht = isht(self.h, self.w, lmax=self.lmax, mmax=self.lmax, grid=sht_grid_type).float()

    def _precompute_channel_groups(self, channel_names, aux_channel_names, n_history=0):
        atmo, surf, dyn_aux, stat_aux, levels = get_channel_groups(channel_names, aux_channel_names)
        sst = [channel_names.index("sst")] if "sst" in channel_names else []
        lsml = [len(channel_names) + aux_channel_names.index("xlsml")] if "xlsml" in aux_channel_names else []
        self.n_atmo_groups = len(levels)
        self.n_atmo_chans = len(atmo) // self.n_atmo_groups
        self.n_surf_chans = len(surf)
        self.n_dyn_aux_chans, self.n_stat_aux_chans = len(dyn_aux), len(stat_aux)
        self.n_aux_chans = self.n_dyn_aux_chans * (n_history + 1) + self.n_stat_aux_chans
        if len(atmo) % self.n_atmo_groups:
            raise ValueError("Expected number of atmospheric variables to be divisible by number of atmospheric groups but got "
                             f"{len(atmo)} and {self.n_atmo_groups}")
        n_dyn = len(atmo) + len(surf) + len(dyn_aux)
        atmo_in, surf_in, sst_in, dyn_aux = list(atmo), list(surf), list(sst), list(dyn_aux)
        for ih in range(1, n_history + 1):
            atmo_in += [c + ih * n_dyn for c in atmo]
            surf_in += [c + ih * n_dyn for c in surf]
            sst_in += [c + ih * n_dyn for c in sst]
            dyn_aux += [c + ih * n_dyn for c in dyn_aux]          # (over the list as grown so far, as in the reference)
        stat_aux = [c + n_history * n_dyn for c in stat_aux]
        for name, idx in (("atmo_channels_in", atmo_in), ("atmo_channels_out", atmo), ("surf_channels_in", surf_in),
                          ("surf_channels_out", surf), ("sst_channels_in", sst_in), ("sst_channels_out", sst),
                          ("dyn_aux_channels", dyn_aux), ("stat_aux_channels", stat_aux), ("land_mask_channels", lsml),
                          ("in_channels", surf_in + atmo_in), ("aux_channels", dyn_aux + stat_aux), ("pred_channels", surf + atmo)):
            self.register_buffer(name, torch.tensor(idx, dtype=torch.long), persistent=False)

    # ---- the reference's stages -------------------------------------------------------------------------------------------------
    def impute_sst_channels(self, x):
        """the composed form: the land mask is sliced out of x and handed over as a tensor"""
        if hasattr(self, "sst_imputation"):
            mask = x[..., self.land_mask_channels, :, :] if self.land_mask_channels.nelement() > 0 else None
            x = self.sst_imputation.impute(x, mask, None)
        return x

    def encode(self, x):
        return self.encoder(x[..., self.in_channels, :, :].contiguous())

    def encode_auxiliary_channels(self, x):
        aux = []
        if hasattr(self, "aux_encoder"):
            aux.append(self.aux_encoder(x[..., self.aux_channels, :, :].contiguous()))
        if hasattr(self, "pos_embed"):
            pos = self.pos_embed()
            lead = aux[0].shape[:-3] if aux else x.shape[:-3]
            aux.append(pos.expand(*lead, *pos.shape[-3:]))          # over the batch: B > 1 works
        return torch.cat(aux, dim=-3) if aux else None

    def decode(self, x):
        return self.decoder(x[..., : self.embed_dim, :, :].contiguous())

    def processor_blocks(self, x, x_aux):
        x = self.pos_drop(x)
        for blk in self.blocks:
            if x_aux is not None:
                x = torch.cat([x, x_aux], dim=-3)
            x = checkpoint(blk, x, use_reentrant=False) if self.checkpointing_level >= 3 else blk(x)
        return x

    def _water_offset(self):
        if hasattr(self, "normalization_means") and hasattr(self, "normalization_stds"):
            return self.normalization_means[self.water_channels] / self.normalization_stds[self.water_channels]
        return None

    def clamp_water_channels(self, x):
        """the composed form"""
        if hasattr(self, "water_channels"):
            off = self._water_offset()
            if off is not None:
                offset = off.view(1, -1, 1, 1).to(x.dtype)
                w = _soft_clamp(x[..., self.water_channels, :, :], offset=offset) - offset
            else:
                w = _soft_clamp(x[..., self.water_channels, :, :])
            x = x.index_copy(-3, self.water_channels, w.to(x.dtype))
        return x

    def _tail_table(self, device):
        """the descriptor of the fused tail, rebuilt when the normalisation buffers change"""
        water = self.water_channels.tolist() if hasattr(self, "water_channels") else []
        off = self._water_offset() if water else None
        key = (device, None if off is None else tuple((b.data_ptr(), b._version) for b in (self.normalization_means, self.normalization_stds)))
        if self._tail.get("key") != key:
            n_x = self.n_in_chans + self.n_aux_chans
            self._tail = dict(key=key, table=ops.tail_table(self.n_out_chans, water, off, self.pred_channels.tolist() if self.big_skip else None,
                                                            n_x, device))
        return self._tail["table"]

    @device_guard
    def forward(self, x):
        if hasattr(self, "sst_imputation"):
            x = self.sst_imputation(x)          # one launch: the land mask is read from the xlsml channel of x itself
        x_in = x
        x_aux = self.encode_auxiliary_channels(x)
        x = checkpoint(self.encode, x, use_reentrant=False) if self.checkpointing_level >= 1 else self.encode(x)
        x = self.processor_blocks(x, x_aux)
        x = checkpoint(self.decode, x, use_reentrant=False) if self.checkpointing_level >= 1 else self.decode(x)
        if not self.big_skip and not hasattr(self, "water_channels"):
            return x
        return ops.Fcn31TailFn.apply(x, x_in if self.big_skip else None, self._tail_table(x.device))          # skip + clamp: one launch
