"""fp64 restatement of what csrc/hydro.hip and ``LossHandler`` compute, written from the definitions in plain torch: the
hydrostatic residual sums and their gradient WRITTEN OUT (no autograd), the outputs of the preparation pass and its backward,
the drift regularization, and the handler's combine (channel weights, multistep weights, running statistics, the weighted
scalar).  It shares no code with ``makani_amd``; the CRPS is the restatement of tests/_crps_ref.py.  Inputs are upcast to fp64
exactly as given (a bf16 input is scored at its bf16 value)."""
import math

import torch

import _crps_ref

Q_MOIST = 0.6078          # makani/utils/constants.py


def quad_weights(H, W):
    """the normalised "naive" rule of an equiangular grid that includes both poles: sin(theta) d theta d lambda over its sum"""
    jac = torch.sin(torch.linspace(0, math.pi, H, dtype=torch.float64)).clamp(min=0.0)
    q = jac[:, None].repeat(1, W)
    return q / q.sum()


# ---- hydrostatic balance ------------------------------------------------------------------------------------------------
def _columns(x, bias, scale, z_idx, t_idx, q_idx):
    """physical Z, dry T, the factor f = 1 + eps q (ones when dry): each (N, K, H, W)"""
    x = x.double()
    b, s = bias.double().reshape(1, -1, 1, 1), scale.double().reshape(1, -1, 1, 1)
    phys = x * s + b
    Z, T = phys[:, z_idx], phys[:, t_idx]
    f = 1.0 + Q_MOIST * phys[:, q_idx] if q_idx else torch.ones_like(T)
    return Z, T, f


def hydro_residuals(x, bias, scale, cmat, z_idx, t_idx, q_idx=None):
    """r (N, K - 1, H, W); the coefficients are the fp32 entries of the loss's ``cmat``, read as they are"""
    Z, T, f = _columns(x, bias, scale, z_idx, t_idx, q_idx)
    cm = cmat.double()
    K = len(z_idx)
    Tv = T * f
    r = []
    for k in range(K - 1):
        pf, hl = cm[k, z_idx[k + 1]], cm[k, t_idx[k]]
        r.append(pf * (Z[:, k + 1] - Z[:, k]) + hl * (Tv[:, k] + Tv[:, k + 1]))
    return torch.stack(r, dim=1)


def hydro_sums(x, bias, scale, cmat, z_idx, t_idx, q_idx, quad, wgt=None):
    """(N, K - 1): sum over the plane of quad w r^2"""
    r = hydro_residuals(x, bias, scale, cmat, z_idx, t_idx, q_idx)
    v = r * r
    if wgt is not None:
        v = v * wgt.double()
    return (v * quad.double()).sum(dim=(-2, -1))


def hydro_grad(x, bias, scale, cmat, z_idx, t_idx, q_idx, quad, g, wgt=None):
    """d sum_{n,k} g[n, k] sums[n, k] / d x, every channel, written out: c_k = 2 g_k quad w r_k;
    d/dZ_k = pf (c_{k-1} - c_k), d/dTv_k = hl_k c_k + hl_{k-1} c_{k-1}; Tv = T f: d/dT = f d/dTv, d/dq_phys = eps T d/dTv"""
    Z, T, f = _columns(x, bias, scale, z_idx, t_idx, q_idx)
    r = hydro_residuals(x, bias, scale, cmat, z_idx, t_idx, q_idx)
    cm, s = cmat.double(), scale.double().reshape(-1)
    K = len(z_idx)
    c = 2.0 * g.double()[:, :, None, None] * quad.double() * r
    if wgt is not None:
        c = c * wgt.double()
    gx = torch.zeros_like(x, dtype=torch.float64)
    zero = torch.zeros_like(c[:, 0])
    for k in range(K):
        ck = c[:, k] if k < K - 1 else zero
        cm1 = c[:, k - 1] if k > 0 else zero
        pf = cm[0, z_idx[1]]
        hl = cm[k, t_idx[k]] if k < K - 1 else 0.0
        hlm = cm[k - 1, t_idx[k - 1]] if k > 0 else 0.0
        gTv = hl * ck + hlm * cm1
        gx[:, z_idx[k]] = s[z_idx[k]] * pf * (cm1 - ck)
        gx[:, t_idx[k]] = s[t_idx[k]] * f[:, k] * gTv
        if q_idx:
            gx[:, q_idx[k]] = s[q_idx[k]] * Q_MOIST * T[:, k] * gTv
    return gx


def hydro_sums_fp32(x, bias, scale, cmat, z_idx, t_idx, q_idx, quad, wgt=None):
    """the reference's formula step by step in plain fp32 torch (de-normalise, moist correction, the matrix product with
    ``cmat``, square, weight, quadrature): the yardstick of the cancelling case"""
    phys = x.float() * scale.float().reshape(1, -1, 1, 1) + bias.float().reshape(1, -1, 1, 1)
    if q_idx:
        phys[:, t_idx] = phys[:, t_idx] * (1.0 + Q_MOIST * phys[:, q_idx])
    N, C, H, W = phys.shape
    r = torch.matmul(cmat.float(), phys.permute(1, 0, 2, 3).reshape(C, -1)).reshape(-1, N, H, W).permute(1, 0, 2, 3)
    v = torch.square(r)
    if wgt is not None:
        v = v * wgt.float()
    return torch.sum(v * quad.float(), dim=(-2, -1))


# ---- the preparation pass -----------------------------------------------------------------------------------------------
def prep(prd, tar, inp, inv=None):
    """prd (B, E, ...), tar, inp (B, ...) -> mean, prd_t, mean_t, tar_t in fp64 (inp / tar may be None)"""
    p = prd.double()
    mean = p.sum(dim=1) * (1.0 / p.shape[1] if inv is None else inv)
    if inp is None:
        return mean, None, None, None
    i = inp.double()
    return mean, p - i[:, None], mean - i, (tar.double() - i if tar is not None else None)


def prep_bwd(E, inv, g_prd_t=None, g_mean=None, g_mean_t=None):
    """g_prd (B, E, ...) = g_prd_t + inv (g_mean + g_mean_t), absent terms skipped"""
    s = 0.0
    for g in (g_mean, g_mean_t):
        if g is not None:
            s = s + g.double()
    s = (s * inv)[:, None] if torch.is_tensor(s) else None
    out = g_prd_t.double() if g_prd_t is not None else 0.0
    if s is not None:
        out = out + s.expand(-1, E, *s.shape[2:])
    return out


# ---- the losses of the recorded handler cases ---------------------------------------------------------------------------
def drift(prd, tar, quad, p):
    """|quadrature(prd) - quadrature(tar)|^p, the mean over the members of a 5-D prediction -> (B, C)"""
    a = (prd.double() * quad.double()).sum(dim=(-2, -1))
    b = (tar.double() * quad.double()).sum(dim=(-2, -1))
    if prd.dim() == 5:
        return (a - b[:, None]).abs().pow(p).mean(dim=1)
    return (a - b).abs().pow(p)


def l2(prd, tar, quad):
    return ((prd.double() - tar.double()).pow(2) * quad.double()).sum(dim=(-2, -1)).sqrt()


_SURFACE_01 = ("u10m", "v10m", "u100m", "v100m", "tp", "sp", "msl", "tcwv", "sst")


def channel_weights(names, kind, time_diff_scale=None):
    """the "constant" and "auto" rules, normalised, times the time-difference scale; fp32 as the handler's buffer is"""
    w = torch.ones(len(names), dtype=torch.float32)
    if kind == "auto":
        for c, n in enumerate(names):
            w[c] = 0.1 if n in _SURFACE_01 else 1.0 if n in ("t2m", "2d") else 0.001 * float(n[1:]) if n[0] in "zuvtrq" else 0.01
    else:
        assert kind == "constant"
    w = w / w.sum()
    return w if time_diff_scale is None else w * time_diff_scale


def levels(names, a, b, p_min, p_max):
    """the shared pressure levels of two variables inside [p_min, p_max], highest pressure first: (indices of a, of b, levels)"""
    pa = {int(n[1:]) for n in names if n[0] == a and n[1:].isdigit()}
    pb = {int(n[1:]) for n in names if n[0] == b and n[1:].isdigit()}
    ps = sorted((p for p in pa & pb if p_min <= p <= p_max), reverse=True)
    return [names.index(f"{a}{p}") for p in ps], [names.index(f"{b}{p}") for p in ps], ps


class Handler:
    """the combine of ``LossHandler`` for the loss types of the recorded cases (l2, ensemble_crps, drift_regularization,
    hydrostatic), in fp64; the buffers are fp32 values as the handler holds them"""

    def __init__(self, meta, bias, scale, tds, cmat=None):
        self.meta, self.names = meta, meta["channel_names"]
        self.S = meta["n_future"] + 1
        self.bias, self.scale, self.cmat = bias, scale, cmat
        self.quad = quad_weights(meta["img_shape_x_resampled"], meta["img_shape_y_resampled"])
        C = len(self.names)
        chw = []
        for loss in meta["losses"]:
            t = None
            if loss.get("temp_diff_normalization", False):
                t = scale.float().flatten() / torch.clamp(tds.float().flatten(), min=1e-4)
            if loss["type"] == "hydrostatic":
                n = len(levels(self.names, "z", "t", loss["parameters"].get("p_min", 0), loss["parameters"].get("p_max", 1000))[2]) - 1
                w = torch.ones(n) / n
            else:
                w = channel_weights(self.names, loss.get("channel_weights", "constant"), t)
            chw.append(w.reshape(1, -1) * loss.get("relative_weight", 1.0))
        self.chw = torch.cat(chw, dim=1)
        ncw = self.chw.shape[1]
        kind = meta.get("multistep", {"weight_type": "constant"})["weight_type"]
        steps = torch.arange(1, self.S + 1, dtype=torch.float32)
        msw = {"constant": torch.ones(self.S) / self.S, "linear": steps / self.S, "balanced": 2.0 * steps / ((self.S + 1) * self.S)}[kind]
        self.msw = msw.reshape(1, -1).repeat_interleave(ncw, dim=1)
        self.mean, self.m2, self.count = torch.zeros(self.S * ncw, dtype=torch.float64), torch.ones(self.S * ncw, dtype=torch.float64), 0
        self.C = C

    def update(self, x):
        """Chan's update of the running mean and second moment with the (B, n) batch x"""
        n = x.shape[0]
        var, mean = torch.var_mean(x.double(), dim=0, correction=0)
        delta = mean - self.mean
        self.m2 = self.m2 + var * n + delta ** 2 * self.count * n / (self.count + n)
        self.mean = self.mean + delta * n / (self.count + n)
        self.count += n

    def vectors(self, prd, tar, inp):
        """the per-loss vectors, each (B, S n_channels) step-major"""
        mean, prd_t, mean_t, tar_t = prep(prd, tar, inp[:, -self.C:] if inp is not None else None)
        out = []
        B = prd.shape[0]
        for loss in self.meta["losses"]:
            tend = loss.get("tendency", False) and inp is not None
            kind = loss["type"]
            if kind == "l2":
                out.append(l2(mean_t if tend else mean, tar_t if tend else tar, self.quad))
            elif kind == "ensemble_crps":
                out.append(_crps_ref.crps(prd_t if tend else prd.double(), tar_t if tend else tar.double(), self.quad))
            elif kind == "drift_regularization":
                out.append(drift(prd_t if tend else prd, tar_t if tend else tar, self.quad, loss["parameters"]["p"]))
            elif kind == "hydrostatic":
                par = loss["parameters"]
                z, t, _ = levels(self.names, "z", "t", par.get("p_min", 0), par.get("p_max", 1000))
                q = levels(self.names, "q", "t", par.get("p_min", 0), par.get("p_max", 1000))[0] if par.get("use_moist_air_formula") else None
                x = (mean_t if tend else mean).reshape(B * self.S, self.C, *mean.shape[-2:])
                out.append(hydro_sums(x, self.bias, self.scale, self.cmat, z, t, q, self.quad).reshape(B, -1))
            else:
                raise NotImplementedError(kind)
        return out

    def __call__(self, prd, tar, inp=None):
        """(scalar, vectors); training cases update the running statistics first, as the handler does"""
        vec = self.vectors(prd, tar, inp)
        allv = torch.cat(vec, dim=-1)
        training = self.meta["training"]
        tracked = self.meta["handler_kwargs"].get("track_running_stats", False) or self.meta.get("balanced_weighting", False)
        if training and tracked:
            self.update(allv.detach())
        chw = self.chw.double()
        if self.meta.get("balanced_weighting", False) and training:
            mean = self.mean if self.count > 100 else torch.ones_like(self.mean)
            chw = chw / (mean + 1e-6)
        if training:
            if self.S > 1:
                chw = chw.repeat(1, self.S)          # the per-loss weights, concatenated, tiled per step (loss.py:488)
            chw = chw * self.msw.double()
        return (chw * allv).sum(dim=1).mean(dim=0), vec


# ---- the recorded cases -------------------------------------------------------------------------------------------------
class Params:
    """a recipe's parameters as the handlers read them: attributes, and ``get`` with a default"""

    def __init__(self, **entries):
        self.__dict__.update(entries)

    def get(self, key, default=None):
        return getattr(self, key, default)


PARAM_KEYS = ("n_future", "n_history", "img_shape_x_resampled", "img_shape_y_resampled", "img_crop_offset_x", "img_crop_offset_y",
              "channel_names", "out_channels", "model_grid_type", "losses", "multistep", "balanced_weighting")


def params_of(meta):
    return Params(**{k: meta[k] for k in PARAM_KEYS if k in meta})


def case_inputs(golden, name, call="R"):
    """(prd, tar, inp | None) of a recorded call, fp32: int8 times 2^-shift"""
    import json
    meta = json.loads(str(golden[f"{name}/meta"]))
    f = 2.0 ** -meta["shift"]
    get = lambda k: torch.from_numpy(golden[f"{name}/call{call}/{k}"].astype("float32")) * f          # noqa: E731
    return get("prd"), get("tar"), (get("inp") if meta["with_inp"] else None)
