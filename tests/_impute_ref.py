"""fp64 restatement of the imputation layers and of the FourCastNet3.1 output tail, written from their formulas with the
gradients derived by hand (numpy, no autograd), plus the reference's torch composition of the same layers in a dtype of the
caller's choice.  tests/test_imputation.py pins the restatement to values recorded from the reference's own classes
(tests/golden/imputation.npz); the GPU tests compare the kernels with the restatement, and use the composition in fp32 as the
yardstick of what plain fp32 arithmetic gives on the same inputs.

Conventions: x (B, C, H, W); imp a list of NI channel indices; mask None or an array broadcastable to (B, NI, H, W) for the MLP
and to x for the constant layer, any nonzero value counts; w1 (hidden, C), b1 (hidden), w2 (NI, hidden)."""
import math

import numpy as np
import torch

ACTS = ("gelu", "relu", "silu", "sin")
_erf = np.vectorize(math.erf, otypes=[np.float64])


def act_pair(h, act):
    """activation and derivative, fp64"""
    if act == "gelu":
        cdf = 0.5 * (1.0 + _erf(h / math.sqrt(2.0)))
        return h * cdf, cdf + h * np.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    if act == "relu":
        return np.where(h > 0, h, 0.0), (h > 0).astype(np.float64)
    if act == "silu":
        s = 1.0 / (1.0 + np.exp(-h))
        return h * s, s * (1.0 + h * (1.0 - s))
    if act == "sin":
        return np.sin(h), np.cos(h)
    raise ValueError(act)


def mlp_mask(x, imp, mask):
    """(B, NI, H, W) bool: NaN in the imputed channels, or flagged"""
    x = np.asarray(x, dtype=np.float64)
    m = np.isnan(x[:, imp])
    if mask is not None:
        m = m | np.broadcast_to(np.asarray(mask) != 0, m.shape)
    return m


def _mlp_parts(x, imp, mask, w1, b1, w2, act):
    x = np.asarray(x, dtype=np.float64)
    w1, b1, w2 = (np.asarray(t, dtype=np.float64) for t in (w1, b1, w2))
    m = mlp_mask(x, imp, mask)
    xc = x.copy()
    xc[:, imp] = np.where(m, 0.0, x[:, imp])
    h = np.einsum("kc,bchw->bkhw", w1, xc) + b1[None, :, None, None]
    a, da = act_pair(h, act)
    o = np.einsum("jk,bkhw->bjhw", w2, a)
    return x, m, xc, a, da, o, w1, w2


def mlp_fwd(x, imp, mask, w1, b1, w2, act="gelu"):
    x, m, xc, _, _, o, _, _ = _mlp_parts(x, imp, mask, w1, b1, w2, act)
    y = xc.copy()
    y[:, imp] = np.where(m, o, xc[:, imp])
    return y


def mlp_bwd(x, g, imp, mask, w1, b1, w2, act="gelu"):
    """(gx, gw1, gb1, gw2) of sum(y * g)"""
    x, m, xc, a, da, _, w1, w2 = _mlp_parts(x, imp, mask, w1, b1, w2, act)
    g = np.asarray(g, dtype=np.float64)
    go = np.where(m, g[:, imp], 0.0)
    gh = np.einsum("jk,bjhw->bkhw", w2, go) * da
    gx = g + np.einsum("kc,bkhw->bchw", w1, gh)
    gx[:, imp] = np.where(m, 0.0, gx[:, imp])
    return gx, np.einsum("bkhw,bchw->kc", gh, xc), gh.sum(axis=(0, 2, 3)), np.einsum("bjhw,bkhw->jk", go, a)


def const_mask(x, mask):
    x = np.asarray(x, dtype=np.float64)
    m = np.isnan(x)
    if mask is not None:
        m = m | np.broadcast_to(np.asarray(mask) != 0, m.shape)
    return m


def const_fwd(x, mask, w):
    m = const_mask(x, mask)
    return np.where(m, np.asarray(w, dtype=np.float64).reshape(1, -1, 1, 1), np.asarray(x, dtype=np.float64))


def const_bwd(x, g, mask):
    """(gx, gw (C))"""
    m = const_mask(x, mask)
    g = np.asarray(g, dtype=np.float64)
    return np.where(m, 0.0, g), np.where(m, g, 0.0).sum(axis=(0, 2, 3))


def soft_clamp(t):
    return np.where(t >= 0.5, t - 0.25, np.where(t > 0, t * t, 0.0))


def soft_clamp_d(t):
    return np.where(t >= 0.5, 1.0, np.where(t > 0, 2.0 * t, 0.0))


def tail_fwd(d, xin, pred, water, off):
    """d (B, Co, H, W); xin (B, Cin, H, W) and pred (Co) or None; water a list of output channels, off one offset each or None"""
    v = np.asarray(d, dtype=np.float64).copy()
    if pred is not None:
        v = v + np.asarray(xin, dtype=np.float64)[:, pred]
    if len(water):
        o = np.zeros(len(water)) if off is None else np.asarray(off, dtype=np.float64)
        o = o.reshape(1, -1, 1, 1)
        v[:, water] = soft_clamp(v[:, water] + o) - o
    return v


def tail_bwd(d, xin, g, pred, water, off):
    """(gd, gxin | None)"""
    v = np.asarray(d, dtype=np.float64).copy()
    if pred is not None:
        v = v + np.asarray(xin, dtype=np.float64)[:, pred]
    gd = np.asarray(g, dtype=np.float64).copy()
    if len(water):
        o = np.zeros(len(water)) if off is None else np.asarray(off, dtype=np.float64)
        gd[:, water] = gd[:, water] * soft_clamp_d(v[:, water] + o.reshape(1, -1, 1, 1))
    if pred is None:
        return gd, None
    gxin = np.zeros(np.asarray(xin).shape, dtype=np.float64)
    gxin[:, pred] = gd
    return gd, gxin


# ---- the reference's composition in torch (makani/models/common/imputation.py:110-129,186-190; fourcastnet3_1.py:61-65,1062-1080) --
def _torch_act(h, act):
    if act == "gelu":
        return torch.nn.functional.gelu(h)
    return {"relu": torch.relu, "silu": torch.nn.functional.silu, "sin": torch.sin}[act](h)


def compose_mlp(x, imp, mask, w1, b1, w2, act="gelu"):
    """slice, isnan, logical_or, where, scatter, two 1x1 convolutions, where, scatter; tensors of one dtype and device"""
    idx = torch.as_tensor(imp, device=x.device)
    x_sub = x[:, idx]
    m = torch.isnan(x_sub) if mask is None else torch.logical_or(mask, torch.isnan(x_sub))
    x_zeroed = torch.where(m, torch.zeros_like(x_sub), x_sub)
    index = idx.view(1, -1, 1, 1).expand_as(x_zeroed)
    x_clean = x.scatter(1, index, x_zeroed)
    h = torch.nn.functional.conv2d(x_clean, w1[:, :, None, None], b1)
    o = torch.nn.functional.conv2d(_torch_act(h, act), w2[:, :, None, None])
    return x_clean.scatter(1, index, torch.where(m, o, x_zeroed))


def compose_const(x, mask, w):
    m = torch.isnan(x) if mask is None else torch.logical_or(mask, torch.isnan(x))
    return torch.where(m, w.view(-1, 1, 1), x)


def compose_tail(d, xin, pred, water, off):
    x = d
    if pred is not None:
        x = x + xin[:, torch.as_tensor(pred, device=d.device)]
    if len(water):
        wi = torch.as_tensor(water, device=d.device)
        o = 0.0 if off is None else off.view(1, -1, 1, 1).to(x.dtype)
        t = x[:, wi] + o
        y = torch.where(t > 0.0, t ** 2, 0.0)
        x = x.index_copy(1, wi, (torch.where(t >= 0.5, t - 0.25, y) - o).to(x.dtype))
    return x
