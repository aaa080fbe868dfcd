"""fp64 restatement of the preprocessing around the network, written from the definition (torch float64 on the CPU, gradients
by torch autograd).  It shares no code with makani_amd: the tests compare the HIP kernels and ``Preprocessor2D`` against it, and
tests/test_preproc.py compares IT against arrays recorded from the reference's own ``Preprocessor2D``.

Per time level the channels are [C data | U unpredicted | N noise], J = C + U + N, T = n_history + 1.
    omega[t, h, w] = wt[t] q[h, w],  sum omega = 1
    mu[b, j]    = sum_{t,h,w} omega v
    sigma[b, j] = sqrt(sum_{t,h,w} omega (v - mu)^2)
    out[b, t J + j] = (v - mu) / sigma,   out[b, T J + s] = static[s]
    y = (yn - bias) sigma[:, :C_out] + mu[:, :C_out]
"""
import math

import torch

F64 = torch.float64


def quad_weights(H, W):
    """normalised quadrature weights of the equiangular grid ("naive" rule): sin(theta) on linspace(0, pi, H), sum 1"""
    jac = torch.clamp(torch.sin(torch.linspace(0, math.pi, H, dtype=F64)), min=0.0)
    q = jac.unsqueeze(1).repeat(1, W)
    return q / q.sum()


def time_weights(mode, n_history, decay=None):
    T = n_history + 1
    if mode == "mean":
        return torch.full((T,), 1.0 / T, dtype=F64)
    if mode == "exponential":
        w = torch.exp(-decay * torch.arange(n_history, -1, -1, dtype=F64))          # the first level is the oldest
        return w / w.sum()
    raise ValueError(mode)


def concat(win, unp, noi, T):
    """(B, T, J, H, W) from the window (B, T C, H, W) and the optional (B, T, U, H, W), (B, T, N, H, W)"""
    B, TC, H, W = win.shape
    parts = [win.reshape(B, T, TC // T, H, W)]
    if unp is not None:
        parts.append(unp)
    if noi is not None:
        parts.append(noi)
    return torch.cat(parts, dim=2)


def stats(x5, q, wt):
    """mu, sigma (B, J) of x5 (B, T, J, H, W)"""
    om = wt.reshape(1, -1, 1, 1, 1) * q.reshape(1, 1, 1, *q.shape[-2:])
    mu = (om * x5).sum(dim=(1, 3, 4))
    var = (om * (x5 - mu[:, None, :, None, None]) ** 2).sum(dim=(1, 3, 4))
    return mu, torch.sqrt(var)


def normalize(x5, mu, sigma):
    return (x5 - mu[:, None, :, None, None]) / sigma[:, None, :, None, None]


def assemble(win, unp, noi, static, T, mode, q=None, wt=None, mu=None, sigma=None):
    """the network input (B, T J + S, H, W) and the statistics (None, None for mode "none"); given mu / sigma are used as they are"""
    x5 = concat(win, unp, noi, T)
    if mode != "none":
        if mu is None:
            mu, sigma = stats(x5, q, wt)
        x5 = normalize(x5, mu, sigma)
    out = x5.flatten(1, 2)
    if static is not None:
        out = torch.cat([out, static.reshape(1, -1, *static.shape[-2:]).expand(out.shape[0], -1, -1, -1)], dim=1)
    return out, mu, sigma


def finish(yn, bias, mu, sigma):
    """bias (C_out, H, W) or None; mu, sigma (B, J) or None (mode "none")"""
    y = yn if bias is None else yn - bias.reshape(1, *bias.shape[-3:])
    if mu is not None:
        c = yn.shape[1]
        y = y * sigma[:, :c, None, None] + mu[:, :c, None, None]
    return y


def append_history(window, pred, T):
    if T == 1:
        return pred
    c = window.shape[1] // T
    return torch.cat([window[:, c:], pred], dim=1)


def slide(unp_inp, unp_tar, step):
    """the cached unpredicted input after rollout step ``step``: the oldest level drops out, the target's level ``step`` comes in"""
    if unp_tar is None or step >= unp_tar.shape[1]:
        return unp_inp
    return torch.cat([unp_inp[:, 1:], unp_tar[:, step:step + 1]], dim=1)


def rollout(model, window, unp_inp, unp_tar, noises, static, bias, T, mode, q, wt, n_future, push_forward=False):
    """the training rollout of the step wrapper: per step assemble -> model -> finish, then the history and the unpredicted cache
    slide.  ``noises``: one (B, T, N, H, W) tensor (or None) per step."""
    result = []
    for step in range(n_future + 1):
        if push_forward:
            window = window.detach()
        x, mu, sigma = assemble(window, unp_inp, noises[step], static, T, mode, q, wt)
        pred = finish(model(x), bias, mu, sigma)
        result.append(pred)
        if step == n_future:
            break
        unp_inp = slide(unp_inp, unp_tar, step) if unp_inp is not None else None
        window = append_history(window, pred, T)
    return torch.cat(result, dim=1)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def seeded(shape, seed, mean=0.0, std=1.0):
    """normals from numpy's frozen legacy stream as float64: the recorder and the tests draw the same inputs from a seed"""
    import numpy as np
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(shape))) * std + mean


def seeded_field(shape, seed, chan_dim=2, ratio=2.0):
    """a field with per-channel sigma in [0.5, 2] and mean +-ratio sigma (no constant channel), rounded to fp32; with ratio 2 the
    quadrature-weighted |mu| / sigma of a 9 x 16 sample stays below 3"""
    import numpy as np
    rs = np.random.RandomState(seed)
    nch = shape[chan_dim]
    view = [1] * len(shape)
    view[chan_dim] = nch
    sigma = torch.from_numpy(0.5 + 1.5 * rs.random_sample(nch)).reshape(view)
    sign = (torch.arange(nch) % 2 * 2 - 1).reshape(view).double()
    x = torch.from_numpy(rs.standard_normal(tuple(shape))) * sigma + ratio * sign * sigma
    return x.float().double()
