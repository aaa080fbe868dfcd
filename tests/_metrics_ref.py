"""fp64 restatement of the seven geometric validation metrics, written from their definitions.  With the quadrature
Q[g] = sum_n q_n w_n g_n over the points of a plane (q the quadrature weights, w optional spatial weights), per sample b and
channel c:

    L1    = Q[|x - y|]                                RMSE = sqrt(R[Q[(x - y)^2]])          (R: the channel / batch reductions)
    ACC   = Q[x'y'] / (sqrt(Q[x'^2] Q[y'^2]) + eps),  x' = x - climatology, y' = y - climatology      ("macro")
            "micro": the three quadratures stacked, the ratio (without eps) is formed after averaging
    with the ensemble mean m_n = 1/E sum_e f_en:
    spread^2 = Q[sum_e (f_e - m)^2] / (E - 1),        skill = Q[(m - o)^2]
    Spread   = sqrt(spread^2),                        SSR = sqrt(spread^2 / max(skill - spread^2 / E, eps))
    rank histogram  H_k = Q[[r = k]],  r_n = #{e : f_en <= o_n},  k = 0 .. E          (members equal to the observation count)
    CRPS: the fair ("skillspread") ensemble CRPS of tests/_crps_ref.py under the normalised quadrature

E = 1 divides 0 by 0 in the spread: NaN, as IEEE arithmetic has it.  Test helper: plain torch, loops over members; shares no code
with the kernels."""
import json
import math

import torch

import _crps_ref


def quadrature_weights(img_shape, normalize=False, crop_shape=None, crop_offset=(0, 0)):
    """equiangular grid: sin(colatitude) weights summing to 4 pi (normalize: to 1) over the whole sphere, then the crop"""
    H, W = img_shape
    theta = torch.linspace(0, math.pi, H, dtype=torch.float64)
    jac = torch.sin(torch.minimum(theta, math.pi - theta)).clamp(min=0.0)          # sin(pi) = 0 exactly, not the rounding of pi
    q = (jac / (jac.sum() * W)).unsqueeze(1).expand(H, W) * (1.0 if normalize else 4.0 * math.pi)
    if crop_shape is not None:
        q = q[crop_offset[0]:crop_offset[0] + crop_shape[0], crop_offset[1]:crop_offset[1] + crop_shape[1]]
    return q


def _wt(q, w, like):
    return (q.double() * (w.double() if w is not None else 1.0)).expand_as(like)


def det_sums(x, y, q, w=None, bias=None):
    """x, y (B, C, H, W), q (H, W), w optional (B, C, H, W), bias optional (C, H, W) -> (B, C, 5):
    Q[|x - y|], Q[(x - y)^2], Q[x'y'], Q[x'^2], Q[y'^2]"""
    x, y = x.double(), y.double()
    wt = _wt(q, w, x)
    a, b = (x - bias.double(), y - bias.double()) if bias is not None else (x, y)
    terms = [(x - y).abs(), (x - y) ** 2, a * b, a * a, b * b]
    return torch.stack([(wt * t).sum(dim=(-2, -1)) for t in terms], dim=-1)


def ens_sums(f, o, q, w=None):
    """f (B, E, C, H, W), o (B, C, H, W) -> (skill (B, C), sum of centred squares (B, C), histogram (B, C, E + 1))"""
    f, o = f.double(), o.double()
    E = f.shape[1]
    wt = _wt(q, w, o)
    m = sum(f[:, e] for e in range(E)) / E
    ss = sum((f[:, e] - m) ** 2 for e in range(E))
    r = sum((f[:, e] <= o).long() for e in range(E))
    hist = torch.stack([(wt * (r == k)).sum(dim=(-2, -1)) for k in range(E + 1)], dim=-1)
    return (wt * (m - o) ** 2).sum(dim=(-2, -1)), (wt * ss).sum(dim=(-2, -1)), hist


def reduce(v, channel_reduction, batch_reduction):
    if channel_reduction != "none":
        v = v.mean(dim=1) if channel_reduction == "mean" else v.sum(dim=1)
    if batch_reduction != "none":
        v = v.mean(dim=0) if batch_reduction == "mean" else v.sum(dim=0)
    return v


def metric(cls, kwargs, a, b, q, w=None, bias=None):
    """the value of class ``cls`` built with ``kwargs`` on (a, b[, w]); q: the quadrature weights of the (cropped) plane"""
    cr, br = kwargs.get("channel_reduction", "mean"), kwargs.get("batch_reduction", "mean")
    if cls in ("GeometricL1", "GeometricRMSE", "GeometricACC"):
        s = det_sums(a, b, q, w, bias)
        if cls == "GeometricL1":
            return reduce(s[..., 0], cr, br)
        if cls == "GeometricRMSE":
            return reduce(s[..., 1], cr, br).sqrt()
        if kwargs.get("method", "macro") == "macro":
            return reduce(s[..., 2] / ((s[..., 3] * s[..., 4]).sqrt() + kwargs.get("eps", 1e-8)), cr, br)
        return reduce(s[..., 2:], cr, br)
    if cls == "GeometricCRPS":
        if a.shape[1] == 1:          # one member: the CRPS of a point forecast is the absolute error
            return reduce(det_sums(a[:, 0], b, q, w)[..., 0], cr, br)
        return reduce(_crps_ref.crps(a, b, q, w, kwargs.get("crps_type", "skillspread")), cr, br)
    E = a.shape[1]
    skill, ss, hist = ens_sums(a, b, q, w)
    if cls == "GeometricRankHistogram":
        return reduce(hist, cr, br)
    var = ss / torch.tensor(float(E - 1), dtype=torch.float64)
    if cls == "GeometricSpread":
        return reduce(var.sqrt(), cr, br)
    if cls == "GeometricSSR":
        return reduce((var / torch.clamp(skill - var / E, min=kwargs.get("eps", 1e-6))).sqrt(), cr, br)
    raise KeyError(cls)


def mismatch(a, b):
    """relative L2 distance of a from b over the entries where b is a number; inf when the NaN patterns differ"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if not torch.equal(torch.isnan(a), torch.isnan(b)):
        return float("inf")
    ok = ~torch.isnan(b)
    den = b[ok].norm().item()
    return (a[ok] - b[ok]).norm().item() / (den if den > 0 else 1.0)


def load_cases(npz):
    """the cases of tests/golden/metrics.npz (tools/make_metrics_golden.py): name -> dict(cls, kwargs, E, a, b, weights | None,
    bias | None, quad_weight, variants: {(channel_reduction, batch_reduction): dict(out, out2[, counts, comb_vals, comb_counts,
    final])}).  Inputs are stored as int8: value = int8 * scale."""
    cases = {}
    for key in npz.files:
        if not key.endswith("/meta"):
            continue
        name = key[:-5]
        meta = json.loads(str(npz[key]))

        def get(k, scale=None):
            if f"{name}/{k}" not in npz.files:
                return None
            t = torch.from_numpy(npz[f"{name}/{k}"])
            return t.float() * scale if scale is not None else t

        variants = {}
        for cr, br in meta["variants"]:
            variants[(cr, br)] = {k: get(f"{cr}-{br}/{k}") for k in ("out", "out2", "counts", "comb_vals", "comb_counts", "final")}
        cases[name] = dict(cls=meta["cls"], kwargs=meta["kwargs"], E=meta["E"], scale=meta["scale"], a=get("a_i8", meta["scale"]),
                           b=get("b_i8", meta["scale"]), weights=get("weights"), bias=get("bias_i8", meta["scale"]),
                           quad_weight=get("quad_weight"), variants=variants)
    return cases
