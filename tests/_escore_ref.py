"""fp64 restatement of the three energy-score losses, written from the definition (Gneiting & Raftery 2007, eq. 22, with the
almost-fair spread factor):

    ES = 1/E sum_e ||o - f_e||^beta  -  (E - 1 + alpha) / (E^2 (E - 1)) sum_{i<j} ||f_i - f_j||^beta

with three norms:  grid Lp      ||x||^p = sum_n q_n w_n |x_n|^p                        (q: quadrature weights, sum 1)
                   Sobolev      ||x||^2 = sum_lm (offset + rw l (l + 1))^fraction c_m |x_lm|^2     (c_0 = 1, c_m = 2)
                   spectral L2  one score per degree l with ||x||_l^2 = sum_m c_m / 4 pi |x_lm|^2, summed over l
x_lm = SHT(x) / sqrt(4 pi).  A norm^p below eps contributes nothing.  Test helper: plain torch, loops over the pairs."""
import math

import torch

from oracle import sht as osht


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    d = torch.linalg.norm((a - b).reshape(-1))
    n = torch.linalg.norm(b.reshape(-1))
    return float(d / n) if float(n) > 0 else float(d)


def _score(f, o, wt, seg_shape, p, beta, alpha, eps, channel_reduction, scale=None):
    """f (B, E, C, *plane), o (B, C, *plane), wt broadcastable to o (already zero where masked).  seg_shape = (): the norm
    sums the whole plane; (L,): the plane is (L, M), one norm per row, the scores of the rows are added.  scale: optional
    per-output-channel factor of the spread (whole-plane form)"""
    B, E = f.shape[:2]
    axes = (-1,) if seg_shape else tuple(range(-(f.dim() - 3), 0))

    def norm_beta(d):
        v = (wt * d.abs().pow(p)).sum(dim=axes)                    # (B, C) or (B, C, L)
        if channel_reduction:
            v = v.sum(dim=1, keepdim=True)
        r = torch.where(v < eps, torch.ones_like(v), v).pow(beta / p)
        return torch.where(v < eps, torch.zeros_like(v), r)

    skill = sum(norm_beta(o - f[:, e]) for e in range(E)) / E
    spread = torch.zeros_like(skill)
    for i in range(E):
        for j in range(i + 1, E):
            spread = spread + norm_beta(f[:, i] - f[:, j])
    if E > 1:
        spread = spread * (E - 1 + alpha) / (E * E * (E - 1))
    if scale is not None:
        spread = spread * scale.double().reshape(1, -1)
    out = skill - spread
    return out.sum(dim=-1) if seg_shape else out


def quadrature_weights(img_shape, grid_type="equiangular"):
    assert grid_type == "equiangular"
    H, W = img_shape
    jac = torch.sin(torch.linspace(0, math.pi, H, dtype=torch.float64)).clamp(min=0.0)
    return (jac / (jac.sum() * W)).unsqueeze(1).expand(H, W)


def lp_energy_score(f, o, img_shape, w=None, p=2.0, beta=1.0, alpha=1.0, eps=1e-6, channel_reduction=True, scale=None):
    """f (B, E, C, H, W), o (B, C, H, W), w optional (B, C, H, W); a NaN observation masks the point, a NaN forecast is 0"""
    f, o = f.double(), o.double()
    wt = quadrature_weights(img_shape).to(f.device) * (w.double() if w is not None else 1.0)
    wt = torch.where(torch.isnan(o), torch.zeros_like(o), wt.expand_as(o))
    f, o = torch.nan_to_num(f, nan=0.0), torch.nan_to_num(o, nan=0.0)
    return _score(f, o, wt, (), p, beta, alpha, eps, channel_reduction, scale)


def _coefficients(f, o, img_shape, lmax, grid_type):
    H, W = img_shape
    band = min((H - 1) // 2 if grid_type == "equiangular" else H - 1, W // 2)
    lmax = band if lmax is None or lmax > band else lmax
    t = osht.RealSHT(H, W, lmax=lmax, mmax=lmax, grid=grid_type).to(f.device)
    fc, oc = t(f.double()) / math.sqrt(4 * math.pi), t(o.double()) / math.sqrt(4 * math.pi)
    bad = torch.isnan(oc.real) | torch.isnan(oc.imag) | (torch.isnan(fc.real) | torch.isnan(fc.imag)).any(dim=1)
    cm = torch.full((lmax,), 2.0, dtype=torch.float64, device=f.device)
    cm[0] = 1.0
    fc = torch.where(torch.isnan(fc.real) | torch.isnan(fc.imag), torch.zeros_like(fc), fc)
    oc = torch.where(torch.isnan(oc.real) | torch.isnan(oc.imag), torch.zeros_like(oc), oc)
    return fc, oc, bad, cm, lmax


def sobolev_energy_score(f, o, img_shape, lmax=None, alpha=1.0, beta=1.0, offset=1.0, fraction=1.0, relative_weight=1.0, eps=1e-6,
                         channel_reduction=True, grid_type="equiangular"):
    fc, oc, bad, cm, lmax = _coefficients(f, o, img_shape, lmax, grid_type)
    l = torch.arange(lmax, dtype=torch.float64, device=f.device)
    wt = (offset + relative_weight * l * (l + 1)).pow(fraction)[:, None] * cm[None, :]
    wt = torch.where(bad, torch.zeros_like(bad, dtype=torch.float64), wt.expand_as(bad))
    return _score(fc, oc, wt, (), 2.0, beta, alpha, eps, channel_reduction)


def spectral_l2_energy_score(f, o, img_shape, lmax=None, alpha=1.0, beta=1.0, eps=1e-6, channel_reduction=True,
                             grid_type="equiangular"):
    fc, oc, bad, cm, lmax = _coefficients(f, o, img_shape, lmax, grid_type)
    wt = (cm / (4 * math.pi))[None, :].expand(lmax, lmax)
    wt = torch.where(bad, torch.zeros_like(bad, dtype=torch.float64), wt.expand_as(bad))
    return _score(fc, oc, wt, (lmax,), 2.0, beta, alpha, eps, channel_reduction)


def reference(cls, kwargs, f, o, w=None, scale=None):
    """dispatch on the class name / constructor kwargs of a fixture case"""
    img = tuple(kwargs["img_shape"])
    common = {k: kwargs[k] for k in ("alpha", "beta", "eps", "channel_reduction") if k in kwargs}
    if cls == "LpEnergyScoreLoss":
        return lp_energy_score(f, o, img, w=w, p=kwargs.get("p", 2.0), scale=scale, **common)
    extra = {k: kwargs[k] for k in ("lmax", "grid_type") if k in kwargs}
    if cls == "SobolevEnergyScoreLoss":
        extra.update({k: kwargs[k] for k in ("offset", "fraction", "relative_weight") if k in kwargs})
        return sobolev_energy_score(f, o, img, **extra, **common)
    if cls == "SpectralL2EnergyScoreLoss":
        return spectral_l2_energy_score(f, o, img, **extra, **common)
    raise KeyError(cls)


def load_cases(npz):
    """the cases of tests/golden/escore_losses.npz (tools/make_escore_golden.py): name -> dict(cls, kwargs, train, forecasts,
    observations, weights | None, lead_time_step | None, out, grad).  Inputs are stored as int8: value = int8 * scale +
    member_offset * (member + 1), -128 = NaN."""
    import json
    cases = {}
    for key in npz.files:
        if not key.endswith("/meta"):
            continue
        name = key[:-5]
        meta = json.loads(str(npz[key]))
        fq, oq = torch.from_numpy(npz[f"{name}/forecasts_i8"]), torch.from_numpy(npz[f"{name}/observations_i8"])
        E = fq.shape[1]
        f = fq.float() * meta["scale"] + meta["member_offset"] * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
        o = torch.where(oq == -128, float("nan"), oq.float() * meta["scale"])
        opt = {k: (torch.from_numpy(npz[f"{name}/{k}"]) if f"{name}/{k}" in npz.files else None) for k in ("weights", "lead_time_step")}
        cases[name] = dict(cls=meta["cls"], kwargs=meta["kwargs"], train=meta["train"], forecasts=f, observations=o,
                           out=torch.from_numpy(npz[f"{name}/out"]), grad=torch.from_numpy(npz[f"{name}/grad"]), **opt)
    return cases


def temper_scale(case):
    """the spread factor of ``spread_temper_steps`` in train mode: max(lead_time_step / steps, 1)"""
    steps = case["kwargs"].get("spread_temper_steps", 0)
    if not (case["train"] and steps > 0 and case["lead_time_step"] is not None):
        return None
    return torch.clamp(case["lead_time_step"].double() / steps, min=1.0)
