"""fp64 restatement of the adjusted MSE, the ensemble Gaussian likelihood and the Gaussian MMD, written from the definitions.

AMSE (Subich et al., arXiv:2501.19374, eq. 6), with the per-degree power P_l(x) = sum_m c_m |x_lm|^2 / 4 pi (c_0 = 1, c_m = 2:
Parseval for a real field, normalised to the unit sphere), the co-spectrum P_l(x, y) = sum_m c_m Re(x_lm conj(y_lm)) / 4 pi and
the coherence coh_l = P_l(x, y) / sqrt(P_l(x) P_l(y) + eps):

    AMSE = sum_l (sqrt P_l(x) - sqrt P_l(y))^2 + 2 max(P_l(x), P_l(y)) (1 - coh_l)

NLL of the observation under N(mu, s2), mu and s2 the ensemble's mean and (biased) variance, s2 >= eps^2:

    NLL = sum_n q_n w_n 1/2 (log s2_n + (o_n - mu_n)^2 / s2_n)

MMD^2 estimate (Dziugaite et al., arXiv:1505.03906) with the kernel k(a, b) = exp(-d(a, b)^2 / 2 sigma) on the distance
d(a, b) = sum_n q_n w_n |a_n - b_n|^beta, points with a NaN observation or member left out, almost-fair spread factor:

    MMD = 1/E sum_e k(o, f_e) - (E - 1 + alpha) / (E^2 (E - 1)) sum_{i<j} k(f_i, f_j)

Test helper: plain torch, loops over members and pairs; shares no code with the kernels."""
import json
import math

import torch

from oracle import sht as osht


def quadrature_weights(img_shape):
    """equiangular grid: sin(colatitude) weights, normalised to sum 1"""
    H, W = img_shape
    jac = torch.sin(torch.linspace(0, math.pi, H, dtype=torch.float64)).clamp(min=0.0)
    return (jac / (jac.sum() * W)).unsqueeze(1).expand(H, W)


def amse(prd, tar, img_shape, grid_type="equiangular", wgt=None, eps=1e-6):
    """prd, tar (B, C, H, W); wgt broadcastable to (B, C, L, M) -> (B, C)"""
    H, W = img_shape
    band = min((H - 1) // 2 if grid_type == "equiangular" else H - 1, W // 2)
    t = osht.RealSHT(H, W, lmax=band, mmax=band, grid=grid_type).to(prd.device)
    x, y = t(prd.double()), t(tar.double())
    cm = torch.full((band,), 2.0, dtype=torch.float64, device=prd.device)
    cm[0] = 1.0
    wt = cm / (4 * math.pi) * (wgt.double() if wgt is not None else 1.0)
    px = (wt * (x.real ** 2 + x.imag ** 2)).sum(-1)
    py = (wt * (y.real ** 2 + y.imag ** 2)).sum(-1)
    pxy = (wt * (x.real * y.real + x.imag * y.imag)).sum(-1)
    coh = pxy / torch.sqrt(px * py + eps)
    per_degree = (px.sqrt() - py.sqrt()) ** 2 + 2 * torch.maximum(px, py) * (1 - coh)
    return per_degree.sum(-1), coh


def ensemble_nll(f, o, q, w=None, eps=1e-6):
    """f (B, E, C, H, W), o (B, C, H, W), q (H, W), w optional (B, C, H, W) -> (B, C); no gradient through an active clamp"""
    f, o = f.double(), o.double()
    E = f.shape[1]
    mu = sum(f[:, e] for e in range(E)) / E
    var = sum((f[:, e] - mu) ** 2 for e in range(E)) / E
    s2 = torch.where(var < eps ** 2, torch.full_like(var, eps ** 2), var)
    nll = 0.5 * (torch.log(s2) + (o - mu) ** 2 / s2)
    wt = q.double() * (w.double() if w is not None else 1.0)
    return (wt * nll).sum(dim=(-2, -1))


def gaussian_mmd(f, o, q, w=None, sigma=1.0, alpha=1.0, beta=2.0, channel_reduction=False):
    """f (B, E, C, H, W), o (B, C, H, W), q (H, W) -> ((B, C) | (B, 1), the list of exponents d^2 / 2 sigma)"""
    f, o = f.double(), o.double()
    E = f.shape[1]
    bad = torch.isnan(o) | torch.isnan(f).any(dim=1)
    wt = (q.double() * (w.double() if w is not None else 1.0)).expand_as(o)
    wt = torch.where(bad, torch.zeros_like(wt), wt)
    f, o = torch.nan_to_num(f, nan=0.0), torch.nan_to_num(o, nan=0.0)
    exponents = []

    def kern(a, b):
        d = (wt * (a - b).abs().pow(beta)).sum(dim=(-2, -1))
        if channel_reduction:
            d = d.sum(dim=1, keepdim=True)
        exponents.append((0.5 * d * d / sigma).detach())
        return torch.exp(-0.5 * d * d / sigma)

    skill = sum(kern(o, f[:, e]) for e in range(E)) / E
    spread = torch.zeros_like(skill)
    for i in range(E):
        for j in range(i + 1, E):
            spread = spread + kern(f[:, i], f[:, j])
    if E > 1:
        spread = spread * (E - 1 + alpha) / (E * E * (E - 1))
    return skill - spread, exponents


def reference(cls, kwargs, a, b, q=None, w=None):
    """dispatch on the class name / constructor kwargs of a case; q None: the fp64 quadrature weights of this file"""
    img = tuple(kwargs["img_shape"])
    if cls == "SpectralAMSELoss":
        return amse(a, b, img, kwargs.get("grid_type", "equiangular"), w, kwargs.get("eps", 1e-6))[0]
    q = quadrature_weights(img).to(a.device) if q is None else q
    if cls == "EnsembleNLLLoss":
        return ensemble_nll(a, b, q, w, kwargs.get("eps", 1e-6))
    if cls == "GaussianMMDLoss":
        return gaussian_mmd(a, b, q, w, **{k: kwargs[k] for k in ("sigma", "alpha", "beta", "channel_reduction") if k in kwargs})[0]
    raise KeyError(cls)


def load_cases(npz):
    """the cases of tests/golden/rest_losses.npz (tools/make_restloss_golden.py): name -> dict(cls, kwargs, a, b, weights | None,
    quad_weight | None, out, grad); a: forecasts (B, E, C, H, W) or prediction (B, C, H, W), b: observations or target.  Inputs
    are stored as int8: value = int8 * scale, -128 = NaN."""
    cases = {}
    for key in npz.files:
        if not key.endswith("/meta"):
            continue
        name = key[:-5]
        meta = json.loads(str(npz[key]))
        aq, bq = torch.from_numpy(npz[f"{name}/a_i8"]), torch.from_numpy(npz[f"{name}/b_i8"])
        opt = {k: (torch.from_numpy(npz[f"{name}/{k}"]) if f"{name}/{k}" in npz.files else None) for k in ("weights", "quad_weight")}
        cases[name] = dict(cls=meta["cls"], kwargs=meta["kwargs"], a=aq.float() * meta["scale"],
                           b=torch.where(bq == -128, float("nan"), bq.float() * meta["scale"]),
                           out=torch.from_numpy(npz[f"{name}/out"]), grad=torch.from_numpy(npz[f"{name}/grad"]), **opt)
    return cases
