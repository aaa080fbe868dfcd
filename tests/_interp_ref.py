"""fp64 restatement of the stochastic-interpolant stepper, written from the definition (torch on the CPU, gradients by torch
autograd).  It shares no code with makani_amd: the tests compare the HIP kernels and ``StochasticInterpolantWrapper`` against it,
and tests/test_interpolant.py compares IT against arrays recorded from the reference's own class.  ``dtype=torch.float32`` evaluates
the same formulas in fp32 torch, operation by operation: the distance to the fp64 evaluation is the formula's own fp32 error on
the given inputs.

    alpha = 1 - s, beta = s^2, sigma = eps (1 - s), gamma = sqrt(s) sigma; d alpha = -1, d beta = 2 s, d sigma = -eps, d gamma = -eps sqrt(s)
    I = alpha x0 + beta x1 + gamma z,  R = d alpha x0 + d beta x1 + d gamma z
    network input [x0 | x | xu | static | s plane]; rows b S' + j
    sampler: x <- x0 + b(x0, x0, s_0) D_0 + sigma(s_0) sqrt(D_0) z_0;  x <- x + bhat(x, s_i) D_i + sqrt(g^2(s_i) D_i) z_i
"""
import math

import torch

F64 = torch.float64


def schedule(eps):
    """the schedule as functions of a tensor s (the generic form: nothing is simplified)"""
    f = dict(alpha=lambda s: 1.0 - s, dalpha=lambda s: -1.0, beta=lambda s: torch.square(s), dbeta=lambda s: 2.0 * s,
             sigma=lambda s: eps * (1.0 - s), dsigma=lambda s: -1.0 * eps)
    f["gamma"] = lambda s: torch.sqrt(s) * f["sigma"](s)
    f["dgamma"] = lambda s: torch.sqrt(s) * f["dsigma"](s)
    return f


def path(x0, x1, z, s, eps, dtype=F64):
    """x0, x1, z (B, C, H, W), s (B, S') -> interpolant and drift (B S', C, H, W)"""
    f = schedule(eps)
    x0, x1, z, s = (t.to(dtype) for t in (x0, x1, z, s))
    sr = s.reshape(*s.shape, 1, 1, 1)
    x0, x1, z = x0.unsqueeze(1), x1.unsqueeze(1), z.unsqueeze(1)
    inter = f["alpha"](sr) * x0 + f["beta"](sr) * x1 + f["gamma"](sr) * z
    drift = f["dalpha"](sr) * x0 + f["dbeta"](sr) * x1 + f["dgamma"](sr) * z
    return inter.flatten(0, 1), drift.flatten(0, 1)


def net_input(x0, x, xu, static, s, has_s=True):
    """[x0 | x | xu | static | s plane] for N rows; xu (N, U, H, W) | None, static (St, H, W) | None, s (N,)"""
    N, _, H, W = x.shape
    parts = [x0, x]
    if xu is not None:
        parts.append(xu.to(x.dtype))
    if static is not None:
        parts.append(static.to(x.dtype).reshape(1, -1, H, W).expand(N, -1, -1, -1))
    if has_s:
        parts.append(s.to(x.dtype).reshape(N, 1, 1, 1).expand(N, 1, H, W))
    return torch.cat(parts, dim=1)


def assemble(x0, x1, z, s, xu, static, eps, has_s=True, dtype=F64):
    """the training call: the network input X (B S', Cin, H, W) and the drift target D (B S', C, H, W)"""
    Sp = s.shape[1]
    inter, drift = path(x0, x1, z, s, eps, dtype)
    rep = lambda t: None if t is None else t.to(dtype).repeat_interleave(Sp, dim=0)
    return net_input(rep(x0), inter, rep(xu), static, s.to(dtype).flatten(), has_s), drift


def gsq(s, eps, foellmer):
    f = schedule(eps)
    sig = f["sigma"](s)
    if not foellmer:
        return torch.square(sig)
    ratio = torch.where(s > 0, s * f["dbeta"](s) / f["beta"](s), 2.0)
    return torch.abs(2.0 * torch.square(sig) * ratio - 2.0 * s * sig * f["dsigma"](s) - torch.square(sig))


def score(x, x0, b, s, eps):
    f = schedule(eps)
    sig, beta, dbeta = f["sigma"](s), f["beta"](s), f["dbeta"](s)
    A = 1.0 / (s * sig * (dbeta * sig - beta * f["dsigma"](s)))
    c = x * dbeta + (beta * f["dalpha"](s) - dbeta * f["alpha"](s)) * x0
    return A * (beta * b - c)


def stub(weight, bias, dtype=F64):
    """the pointwise network Conv2d(Cin, C, 1) as a function of the input (and, time-aware, the time it ignores)"""
    w, b = weight.to(dtype).reshape(weight.shape[0], -1), bias.to(dtype)
    return lambda x, s=None: torch.einsum("oc,nchw->nohw", w, x) + b.reshape(1, -1, 1, 1)


def sampler(net, x0, xu, static, noises, n_steps, eps, foellmer, time_aware=False, dtype=F64):
    """the SDE sampler; noises: n_steps fields (B, C, H, W)"""
    x0 = x0.to(dtype)
    B = x0.shape[0]
    sig = schedule(eps)["sigma"]
    st = torch.linspace(0, 1, n_steps + 1, dtype=dtype)
    ds = st[1:] - st[:-1]

    def call(x, si):
        sv = si.expand(B)
        xin = net_input(x0, x, xu, static, sv, has_s=not time_aware)
        return net(xin, sv.unsqueeze(1)) if time_aware else net(xin)

    x = x0 + call(x0, st[0]) * ds[0]
    x = x + sig(st[0]) * torch.sqrt(ds[0]) * noises[0].to(dtype)
    for i in range(1, n_steps):
        b = call(x, st[i])
        if foellmer:
            b = b + 0.5 * (gsq(st[i], eps, True) - torch.square(sig(st[i]))) * score(x, x0, b, st[i], eps)
        x = x + b * ds[i]
        x = x + torch.sqrt(gsq(st[i], eps, foellmer) * ds[i]) * noises[i].to(dtype)
    return x


def generic_coefficients(s, ds, eps, foellmer, first):
    """(cx, cb, c0, cn) of x <- cx x + cb b + c0 x0 + cn z from the generic formulas above, evaluated with the schedule functions in
    fp64: bhat = b + k (beta b - d beta x - (beta d alpha - d beta alpha) x0), k = (g^2 - sigma^2) A / 2"""
    f = schedule(eps)
    s, ds = torch.tensor(s, dtype=F64), torch.tensor(ds, dtype=F64)
    sig = f["sigma"](s)
    if first or not foellmer:
        cn = sig * torch.sqrt(ds) if first else torch.sqrt(gsq(s, eps, False) * ds)
        return 1.0, float(ds), 0.0, float(cn)
    beta, dbeta = f["beta"](s), f["dbeta"](s)
    A = 1.0 / (s * sig * (dbeta * sig - beta * f["dsigma"](s)))
    k = 0.5 * (gsq(s, eps, True) - torch.square(sig)) * A
    cx = 1.0 - ds * k * dbeta
    cb = ds * (1.0 + k * beta)
    c0 = -ds * k * (beta * f["dalpha"](s) - dbeta * f["alpha"](s))
    return float(cx), float(cb), float(c0), float(torch.sqrt(gsq(s, eps, True) * ds))


def ulp32(t):
    m = float(t.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 0.0


def bf16_neighbours_ok(got, want64):
    """``got`` (bf16) equals the fp64 value rounded to bf16, or is its neighbour (one bf16 step of the value's binade)"""
    want = want64.to(torch.bfloat16)
    g, w = got.double(), want.double()
    step = torch.where(w != 0, 2.0 ** (torch.floor(torch.log2(w.abs().clamp_min(1e-300))) - 7), torch.zeros_like(w))
    return bool(((g - w).abs() <= step * (1 + 1e-12)).all())


def load_cases(npz):
    """{case: {"meta": dict, key: tensor}} of tests/golden/interpolant.npz"""
    import json
    cases = {}
    for key in npz.files:
        name, field = key.split("/", 1)
        c = cases.setdefault(name, {})
        c[field] = json.loads(str(npz[key])) if field == "meta" else torch.from_numpy(npz[key])
    return cases


def case_inputs(case):
    """the inputs of a fixture case in float32: x0, x1 (B, C, H, W), xu (B, 1, U, H, W) | None from their seeds, and the recorded
    static planes (1, St, H, W) | None (the reference's own linear grid)"""
    from _preproc_ref import seeded
    meta = case["meta"]
    B, C, U, H, W = (meta[k] for k in ("B", "C", "U", "H", "W"))
    sd = meta["seeds"]
    x0 = seeded((B, C, H, W), sd["x0"]).float()
    x1 = seeded((B, C, H, W), sd["x1"]).float()
    xu = seeded((B, 1, U, H, W), sd["xu"]).float() if U else None
    return x0, x1, xu, case.get("static")
