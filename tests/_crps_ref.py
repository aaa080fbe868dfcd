"""fp64 restatement of the ensemble CRPS forms of csrc/crps.hip, written from the definitions in plain torch: one per-point
score and the weighted plane sum  out[b, c] = sum_p q[p] w[b, c, p] s[b, c, p].  Inputs are upcast to fp64 exactly as given
(a bf16 input is scored at its bf16 value); gradients come from autograd.

  "skillspread"        mean_e |f_e - o| - (E - 1 + alpha) / (E^2 (E - 1)) sum_r (2 r - E - 1) f_(r),   f_(1) <= ... <= f_(E)
  "probability weighted moment"   the same with alpha = 1
  "naive skillspread"  the same value with the spread written as sum_{i<j} |f_i - f_j|
  "cdf"                sum_r w_(r) |f_(r) - o| - sum_{i<j} w_(i) w_(j) (f_(j) - f_(i)),   member weights w normalised to sum 1
  "gauss"              sigma (z erf(z / sqrt 2) + 2 phi(z) - 1 / sqrt pi),   z = (o - mu) / sigma,   sigma = max(population std, eps)
  complex members      mean_e |o - f_e| - (E - 1 + alpha) / (E^2 (E - 1)) sum_{i<j} |f_i - f_j|   with the complex modulus

The order statistics come from ``torch.sort(dim=1, stable=True)``: autograd through the stable sort hands tied members the
rank-order gradient (the earlier member takes the lower rank), which is the operation's definition for the sorted forms; in
the pairwise forms a tied pair contributes nothing to the gradient (torch's derivative of |x| at 0 is 0, real and complex).
A NaN observation masks the point (score 0, zero gradient) in the skillspread, PWM, naive and complex forms; "cdf" and
"gauss" do not mask, a NaN observation gives a NaN score.  Test helper."""
import math

import torch

MASKING = ("skillspread", "probability weighted moment", "naive skillspread")


def _pair_spread(f):
    """sum_{i<j} |f_i - f_j| over the member axis 1 (real or complex), one member at a time"""
    E = f.shape[1]
    tot = torch.zeros_like(f[:, 0].abs())
    for i in range(E - 1):
        tot = tot + (f[:, i:i + 1] - f[:, i + 1:]).abs().sum(dim=1)
    return tot


def point_score(f, o, crps_type, alpha=1.0, eps=1.0e-6, ens_w=None):
    """f (B, E, C, *plane), o (B, C, *plane), fp64 / complex128 -> the score of every point (B, C, *plane).  Complex members
    take the complex naive form whatever ``crps_type`` says."""
    E = f.shape[1]
    if crps_type == "probability weighted moment" and not f.is_complex():
        alpha = 1.0
    fair = (E - 1 + alpha) / (E * E * (E - 1))
    if f.is_complex():
        masked = torch.isnan(o.real) | torch.isnan(o.imag)
        o0 = torch.where(masked, torch.zeros_like(o), o)
        s = (o0.unsqueeze(1) - f).abs().mean(dim=1) - fair * _pair_spread(f)
        return torch.where(masked, torch.zeros_like(s), s)
    if crps_type in MASKING:
        masked = torch.isnan(o)
        o0 = torch.where(masked, torch.zeros_like(o), o)
        skill = (f - o0.unsqueeze(1)).abs().mean(dim=1)
        if crps_type == "naive skillspread":
            spread = _pair_spread(f)
        else:
            fs, _ = torch.sort(f, dim=1, stable=True)
            r = torch.arange(1, E + 1, dtype=f.dtype, device=f.device).reshape(1, E, *([1] * (f.dim() - 2)))
            spread = ((2 * r - E - 1) * fs).sum(dim=1)
        s = skill - fair * spread
        return torch.where(masked, torch.zeros_like(s), s)
    if crps_type == "cdf":
        w = torch.ones(E, dtype=f.dtype, device=f.device) if ens_w is None else ens_w.to(f.device, f.dtype)
        w = w / w.sum()
        fs, idx = torch.sort(f, dim=1, stable=True)
        ws = w[idx]
        cum = torch.cumsum(ws, dim=1)
        # sum_{i<j} w_i w_j (f_j - f_i) = sum_r w_r f_r (W_{<r} - W_{>r}),   W_{<r} = cum_r - w_r,   W_{>r} = 1 - cum_r
        return (ws * (fs - o.unsqueeze(1)).abs()).sum(dim=1) - (ws * fs * (2 * cum - ws - 1)).sum(dim=1)
    if crps_type == "gauss":
        mu = f.mean(dim=1)
        sigma = torch.clamp(torch.sqrt(((f - mu.unsqueeze(1)) ** 2).mean(dim=1)), min=eps)
        z = (o - mu) / sigma
        phi = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
        return sigma * (z * torch.erf(z / math.sqrt(2)) + 2 * phi - 1 / math.sqrt(math.pi))
    raise KeyError(crps_type)


def crps(f, o, q, w=None, crps_type="skillspread", alpha=1.0, eps=1.0e-6, ens_w=None):
    """f (B, E, C, *plane), o (B, C, *plane), q (points of a plane, any shape), w optional, broadcastable to o -> (B, C) fp64"""
    cplx = f.is_complex() or o.is_complex()
    f, o = (f.to(torch.complex128), o.to(torch.complex128)) if cplx else (f.double(), o.double())
    s = point_score(f, o, crps_type, alpha, eps, ens_w).flatten(2)
    wt = q.double().reshape(1, 1, -1).to(s.device)
    if w is not None:
        wt = wt * w.double().expand(o.shape).flatten(2)
    return (wt * s).sum(dim=-1)
