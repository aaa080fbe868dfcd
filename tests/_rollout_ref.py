"""fp64 restatement of the rollout diagnostics (``makani/utils/inference/rollout_buffer.py:670-1338``) and the inputs the tests of
``makani_amd.rollout_buffer`` share.

* ``restatement(kind, updates, ...)``: the three ``update`` sequences in fp64 — de-normalise, transform (``oracle/sht.py`` in fp64
  for the spectrum, ``torch.fft`` in fp64 for the zonal spectrum), weight, sum — and the statistics POOLED over every sample of
  every update in two passes (mean first, then the centred squares).  ``finalize_ref`` is ``std = sqrt(M2 / (n - 1))``.
* ``reference_sequence(kind, updates, ...)``: the reference's own op sequence in fp32 torch — ``scale * x + bias``, the oracle SHT
  or ``torch.fft.rfft`` in fp32, ``var_mean`` over the batch, ``_welford_combine`` with ``float(count)`` — update by update.  What
  it misses against the restatement is the floor of the fp32 formula on these inputs.
* ``CASES`` and ``make_updates``: grids, channel selections, ensemble sizes, dtypes and affine maps of the GPU tests.
"""
import math
import os
import sys
import zlib
from functools import lru_cache

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import sht as osht  # noqa: E402

BATCHES = (2, 3, 1)          # three successive updates; the last has zero batch M2, the first starts from n0 = 0
T, IDT = 3, 1                # lead-time slots and the one the updates go to
GATE_F32, GATE_BF16 = 1e-5, 2.0 ** -8

# name: (nlat, nlon, grid, channels in, selected channels or None = all in order, ensemble size, dtype, affine)
# affine: "none" (no scale / bias), "unit" (bias / scale of order 1), "big" (|bias| = 1e3 scale)
CASES = {
    "9x14-all-e1-f32-none": (9, 14, "equiangular", 5, None, 1, torch.float32, "none"),
    "9x14-sel-e2-f32-unit": (9, 14, "legendre-gauss", 5, ["c3", "c0"], 2, torch.float32, "unit"),
    "9x14-6of7-e4-bf16-unit": (9, 14, "equiangular", 7, ["c0", "c1", "c2", "c4", "c5", "c6"], 4, torch.bfloat16, "unit"),
    "9x14-25ch-e4-f32-unit": (9, 14, "equiangular", 25, None, 4, torch.float32, "unit"),      # 112 member rows: three zonal row tiles
    "17x32-all-e2-f32-unit": (17, 32, "equiangular", 5, None, 2, torch.float32, "unit"),
    "17x32-6of7-e4-f32-unit": (17, 32, "legendre-gauss", 7, ["c0", "c1", "c2", "c4", "c5", "c6"], 4, torch.float32, "unit"),
    "17x32-all-e1-bf16-none": (17, 32, "legendre-gauss", 5, None, 1, torch.bfloat16, "none"),
    "17x32-sel-e2-f32-big": (17, 32, "equiangular", 5, ["c3", "c0"], 2, torch.float32, "big"),
    "91x180-all-e1-f32-unit": (91, 180, "equiangular", 5, None, 1, torch.float32, "unit"),
    "91x180-sel-e2-bf16-unit": (91, 180, "equiangular", 5, ["c3", "c0"], 2, torch.bfloat16, "unit"),
}


def names(n):
    return [f"c{i}" for i in range(n)]


def latitudes(nlat):
    """latitudes in degrees, north to south (what ``lat_lon[0]`` holds)"""
    return np.linspace(90.0, -90.0, nlat).tolist()


def longitudes(nlon):
    return np.linspace(0.0, 360.0, nlon, endpoint=False).tolist()


def affine(kind, nchan):
    """(scale, bias) over ALL input channels in the reference's (1, C, 1, 1) shape, or (None, None)"""
    if kind == "none":
        return None, None
    c = torch.arange(nchan, dtype=torch.float32)
    scale = 0.5 + 0.25 * c
    sign = 1.0 - 2.0 * (c % 2)
    bias = sign * scale * (1e3 if kind == "big" else (0.6 + 0.1 * c))
    return scale.reshape(1, -1, 1, 1), bias.reshape(1, -1, 1, 1)


def make_updates(nlat, nlon, nchan, E, dtype, kind="unit", seed=0):
    """[(data (B, E, C, H, W), targ (B, 1, C, H, W))] for B in BATCHES.  Every sample is its own amplitude factor 1 + 0.5 g
    (g: the sample's index over all updates) on a smooth field common to all samples plus noise of its own, so the
    between-sample standard deviation of every statistic is of the order of its mean and the comparison does not measure
    cancellation.  The "big" case multiplies the fields by 40 (|bias| is then 25 field magnitudes): the degree-0 / order-0 power,
    which the bias dominates, still varies between samples by far more than the rounding of one fp32 value, and the fp32
    transform of ``scale * x + bias`` — the reference formula — keeps five digits of the other orders."""
    g = torch.Generator().manual_seed(1000 + seed)
    lat = torch.deg2rad(torch.tensor(latitudes(nlat), dtype=torch.float64))[:, None]
    lon = torch.deg2rad(torch.tensor(longitudes(nlon), dtype=torch.float64))[None, :]
    c = torch.arange(nchan, dtype=torch.float64)[:, None, None]
    smooth = (1.0 + 0.2 * c) * (0.8 + torch.cos(lat) * torch.sin(2 * lon + 0.3 * c) + 0.5 * torch.sin(lat) * torch.cos(lon)
                                + 0.3 * torch.cos(3 * lat) * torch.cos(3 * lon))
    field_scale = 40.0 if kind == "big" else 1.0
    out, seen = [], 0
    for B in BATCHES:
        amp = (1.0 + 0.5 * torch.arange(seen, seen + B, dtype=torch.float64))[:, None, None, None, None]
        seen += B
        noise = 0.3 * torch.randn((B, E + 1, nchan, nlat, nlon), generator=g, dtype=torch.float64)
        member = 1.0 + 0.1 * torch.arange(E + 1, dtype=torch.float64)[None, :, None, None, None]
        x = (field_scale * amp * member * (smooth[None, None] + noise)).to(dtype)
        out.append((x[:, 1:].contiguous(), x[:, :1].contiguous()))
    return out


def mask_of(nchan, selected):
    return list(range(nchan)) if selected is None else [names(nchan).index(s) for s in selected]


@lru_cache(maxsize=None)
def oracle_sht(nlat, nlon, grid):
    return osht.RealSHT(nlat, nlon, grid=grid)


def lat_weights(nlat):
    """cos(latitude) as the reference forms it (fp32 on the device)"""
    return torch.cos(torch.deg2rad(torch.tensor(latitudes(nlat), dtype=torch.float32)))


def _statistic(kind, data, targ, mask, scale, bias, nlat, nlon, grid, work, in_dtype):
    """the per-sample statistic of one update in ``work`` precision: temporal (B, C, H, W), spectrum (B, C, E1, L),
    zonal (B, C, E1, H, M)"""
    C = len(mask)
    s = scale.reshape(-1)[mask].to(work) if scale is not None else torch.ones(C, dtype=work)
    o = bias.reshape(-1)[mask].to(work) if bias is not None else torch.zeros(C, dtype=work)
    if kind == "temporal":
        return s.reshape(1, -1, 1, 1) * data[:, 0][:, mask].to(work) + o.reshape(1, -1, 1, 1)
    x = torch.cat([targ, data], dim=1)[:, :, mask].to(work)
    x = s.reshape(1, 1, -1, 1, 1) * x + o.reshape(1, 1, -1, 1, 1)
    if kind == "spectrum":
        p = torch.square(torch.abs(oracle_sht(nlat, nlon, grid)(x)))
        p[..., 1:] *= 2.0
        p = torch.sum(p, dim=-1)
        p = p.to(in_dtype).to(work)                             # spect.to(dtype): a rounding for bf16 inputs only
        return p.permute(0, 2, 1, 3).contiguous()
    if kind == "zonal":
        f = torch.fft.rfft(x, dim=-1, norm="forward")
        p = lat_weights(nlat).to(work).reshape(1, 1, 1, -1, 1) * torch.square(torch.abs(f))
        p[..., 1:] *= 2.0
        p = p.to(in_dtype).to(work)
        return p.permute(0, 2, 1, 3, 4).contiguous()
    raise ValueError(kind)


def restatement(kind, updates, mask, scale, bias, nlat, nlon, grid):
    """(mean, M2, n) in fp64, pooled over all samples of all updates in two passes"""
    in_dtype = updates[0][0].dtype
    y = torch.cat([_statistic(kind, d, t, mask, scale, bias, nlat, nlon, grid, torch.float64, in_dtype) for d, t in updates], dim=0)
    mean = y.mean(dim=0)
    return mean, torch.square(y - mean[None]).sum(dim=0), y.shape[0]


def finalize_ref(mean, m2, n):
    return mean, torch.sqrt(m2 / (n - 1.0)) if n > 1 else torch.sqrt(m2 / 0.0)


def reference_sequence(kind, updates, mask, scale, bias, nlat, nlon, grid):
    """(running_mean, running_var, n) of the reference's fp32 op sequence, update by update (``:735-753``)"""
    in_dtype = updates[0][0].dtype
    mean = m2 = None
    n = 0
    for d, t in updates:
        y = _statistic(kind, d, t, mask, scale, bias, nlat, nlon, grid, torch.float32, in_dtype)
        count = y.shape[0]
        var, mu = torch.var_mean(y, dim=0, correction=0, keepdim=False)
        if mean is None:
            mean, m2 = torch.zeros_like(mu), torch.zeros_like(mu)
        new = n + count
        delta = mu - mean
        mean = mean + delta * float(count) / float(new)
        m2 = m2 + var * count + torch.square(delta) * float(n * count) / float(new)
        n = new
    return mean, m2, n


def rel(a, b):
    """relative L2 error of ``a`` against ``b``; 0 when both are exactly zero"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.norm().item()
    num = (a - b).norm().item()
    return 0.0 if num == 0.0 else num / max(den, 1e-300)


def split_errors(kind, affine_kind, got, want):
    """{label: relative L2}: one figure per output, or — for the spectral buffers of the "big" case — the degree / order 0 column
    and the rest separately"""
    if affine_kind == "big" and kind in ("spectrum", "zonal"):
        return {"0": rel(got[..., :1], want[..., :1]), "rest": rel(got[..., 1:], want[..., 1:])}
    return {"all": rel(got, want)}


def case_setup(name):
    nlat, nlon, grid, nchan, selected, E, dtype, kind = CASES[name]
    scale, bias = affine(kind, nchan)
    updates = make_updates(nlat, nlon, nchan, E, dtype, kind, seed=zlib.crc32(name.encode()) % 10000)
    return dict(nlat=nlat, nlon=nlon, grid=grid, nchan=nchan, selected=selected, E=E, dtype=dtype, kind=kind, scale=scale, bias=bias,
                updates=updates, mask=mask_of(nchan, selected), gate=GATE_BF16 if dtype == torch.bfloat16 else GATE_F32)
