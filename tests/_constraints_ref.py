"""fp64 restatement of the three output constraints and of their gradients, taking the operators (the buffers the classes
build) as given.  Pinned against the reference's own classes by tests/test_constraints.py (tests/golden/constraints.npz, recorded
by tools/make_constraints_golden.py); the GPU tests compare the kernels with it.

Every function works in (B, C, H, W) layout on the device of ``x``, in ``dtype`` (float64 unless told otherwise: float32 gives
"the reference's formula in plain fp32 torch", whose distance from the fp64 evaluation is the reference's own error on an input);
``buf`` maps buffer names to tensors, ``meta`` is the case's JSON record (index lists, flags, scalars).  The forward functions are
differentiable torch code; the backward functions are the gradients written out, not autograd."""
import math

import torch

Q_EPS = 0.6078          # makani/utils/constants.py: Q_CORRECTION_MOIST_AIR
R_DRY = 287.052874247          # R_DRY_AIR


def _c(t, like):
    return torch.as_tensor(t).to(device=like.device, dtype=like.dtype)


# ---- _HydrostaticBalanceWrapper ---------------------------------------------------------------------------------------------
def wrapper_fwd(x, buf, meta, dtype=torch.float64):
    x = x.to(dtype)
    L, moist = len(meta["z_idx"]), meta["moist"]
    M, isc, ibi, osc, obi = (_c(buf[k], x) for k in ("mapping", "inp_scale", "inp_bias", "out_scale", "out_bias"))
    u = x * isc + ibi
    if moist:
        u = torch.cat([u[:, :1] * (1.0 + Q_EPS * u[:, L + 1: L + 2]), u[:, 1:]], dim=1)
    v = torch.einsum("oc,bchw->bohw", M, u)
    if moist:          # (out of place, so that autograd can run through it; a division by exactly 1 changes nothing)
        t_idx = torch.as_tensor(meta["t_idx"], device=x.device)
        v = v / torch.ones_like(v).index_copy(1, t_idx, 1.0 + Q_EPS * v[:, meta["q_idx"]])
    return (v - obi) / osc


def wrapper_bwd(x, g, buf, meta, dtype=torch.float64):
    """d sum(g * wrapper_fwd(x)) / dx, written out"""
    x, g = x.to(dtype), g.to(dtype)
    L, moist = len(meta["z_idx"]), meta["moist"]
    M, isc, ibi, osc = (_c(buf[k], x) for k in ("mapping", "inp_scale", "inp_bias", "out_scale"))
    t_idx, q_idx = meta["t_idx"], meta.get("q_idx")
    gw = g / osc
    if not moist:
        return torch.einsum("oc,bohw->bchw", M, gw) * isc
    u = x * isc + ibi
    f0 = 1.0 + Q_EPS * u[:, L + 1]
    ut = u.clone()
    ut[:, 0] = u[:, 0] * f0
    v = torch.einsum("oc,bchw->bohw", M, ut)
    f = 1.0 + Q_EPS * v[:, q_idx]          # (B, L, H, W): the output's physical humidity
    gv = gw.clone()
    gv[:, t_idx] = gw[:, t_idx] / f
    gv[:, q_idx] = gw[:, q_idx] - Q_EPS * gw[:, t_idx] * v[:, t_idx] / f ** 2
    gut = torch.einsum("oc,bohw->bchw", M, gv)
    gu = gut.clone()
    gu[:, 0] = gut[:, 0] * f0
    gu[:, L + 1] = gu[:, L + 1] + Q_EPS * gut[:, 0] * u[:, 0]
    return gu * isc


# ---- HydrostaticBalanceProjection -------------------------------------------------------------------------------------------
def projection_fwd(x, buf, meta, dtype=torch.float64):
    x = x.to(dtype)
    idx, L, lam, moist = meta["channel_indices"], meta["num_levels"], meta["strength"], meta["moist"]
    P, off, s, b = _c(buf["proj"], x), _c(buf["off"], x), _c(buf["scale_sub"], x), _c(buf["bias_sub"], x)
    xp = x[:, idx] * s + b
    if moist:
        mult = torch.ones_like(xp)
        mult[:, :L] = 1.0 + Q_EPS * (x[:, meta["q_indices"]] * _c(buf["q_scale"], x) + _c(buf["q_bias"], x))
        xp = xp * mult
    xp = xp - lam * (torch.einsum("oc,bchw->bohw", P, xp) - off)
    if moist:
        xp = xp / mult
    out = x.clone()
    out[:, idx] = (xp - b) / s
    return out


def projection_bwd(x, g, buf, meta, dtype=torch.float64):
    x, g = x.to(dtype), g.to(dtype)
    idx, L, lam, moist = meta["channel_indices"], meta["num_levels"], meta["strength"], meta["moist"]
    P, off, s, b = _c(buf["proj"], x), _c(buf["off"], x), _c(buf["scale_sub"], x), _c(buf["bias_sub"], x)
    gx = g.clone()
    gw = g[:, idx] / s
    if not moist:
        gx[:, idx] = (gw - lam * torch.einsum("oc,bohw->bchw", P, gw)) * s
        return gx
    qs = _c(buf["q_scale"], x)
    mult = torch.ones_like(gw)
    mult[:, :L] = 1.0 + Q_EPS * (x[:, meta["q_indices"]] * qs + _c(buf["q_bias"], x))
    u = x[:, idx] * s + b
    ut = u * mult
    v = ut - lam * (torch.einsum("oc,bchw->bohw", P, ut) - off)
    gv = gw / mult
    gmult = -gv * v / mult
    gut = gv - lam * torch.einsum("oc,bohw->bchw", P, gv)
    gmult = gmult + gut * u
    gx[:, idx] = gut * mult * s
    gx[:, meta["q_indices"]] = gx[:, meta["q_indices"]] + Q_EPS * qs * gmult[:, :L]
    return gx


# ---- NonNegativeConstraint --------------------------------------------------------------------------------------------------
def _softplus(t):
    """``F.softplus`` as the reference calls it: beyond its default threshold of 20 it returns t itself (it drops
    log1p(exp(-t)) <= 2.1e-9 there, far below fp32 resolution of t > 20 but not below the 1e-12 of the CPU pin)"""
    return torch.where(t > 20.0, t, torch.clamp(t, min=0.0) + torch.log1p(torch.exp(-t.abs())))


def nonneg_fwd(x, buf, meta, dtype=torch.float64):
    x = x.to(dtype)
    idx, eps, leak, mode = meta["channel_indices"], meta["eps"], meta["leak"], meta["mode"]
    off = _c(buf["offset"], x) if "offset" in buf else torch.zeros(1, len(idx), 1, 1, dtype=dtype, device=x.device)
    w = x[:, idx]
    if meta["training"]:
        ws = w + off
        if mode == "silu":
            w = ws * torch.sigmoid(ws / eps)
        else:
            w = leak * ws + (1.0 - leak) * eps * (_softplus(ws / eps) - math.log(2.0))
        w = w - off
    else:
        w = torch.maximum(w, -off.expand_as(w))
    out = x.clone()
    out[:, idx] = w
    return out


def nonneg_bwd(x, g, buf, meta, dtype=torch.float64):
    x, g = x.to(dtype), g.to(dtype)
    idx, eps, leak, mode = meta["channel_indices"], meta["eps"], meta["leak"], meta["mode"]
    off = _c(buf["offset"], x) if "offset" in buf else torch.zeros(1, len(idx), 1, 1, dtype=dtype, device=x.device)
    w = x[:, idx]
    if meta["training"]:
        t = (w + off) / eps
        sg = torch.sigmoid(t)
        if mode == "silu":
            d = sg + t * sg * torch.sigmoid(-t)
        else:
            d = leak + (1.0 - leak) * torch.where(t > 20.0, torch.ones_like(sg), sg)          # (the threshold of _softplus)
    else:
        d = (w >= -off).to(dtype)
    gx = g.clone()
    gx[:, idx] = g[:, idx] * d
    return gx


FWD = {"wrapper": wrapper_fwd, "projection": projection_fwd, "nonneg": nonneg_fwd}
BWD = {"wrapper": wrapper_bwd, "projection": projection_bwd, "nonneg": nonneg_bwd}


def load_cases(npz):
    """{case: {"meta": dict, "buf": {name: tensor}, "<array>": tensor}} of tests/golden/constraints.npz"""
    import json
    cases = {}
    for key in npz.files:
        name, rest = key.split("/", 1)
        c = cases.setdefault(name, {"buf": {}})
        if rest == "meta":
            c["meta"] = json.loads(str(npz[key]))
        elif rest.startswith("buf/"):
            c["buf"][rest[4:]] = torch.from_numpy(npz[key])
        else:
            c[rest] = torch.from_numpy(npz[key])
    return cases
