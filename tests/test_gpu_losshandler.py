"""``mk_hydro_sums`` / ``mk_hydro_grad``, ``mk_loss_prep_fwd`` / ``mk_loss_prep_bwd``, ``DriftRegularization`` and ``LossHandler`` on
the GPU against the fp64 restatement of tests/_losshandler_ref.py (pinned to the reference's recorded values by
tests/test_losshandler.py) and against those recorded values themselves (tests/golden/losshandler.npz).

Gates, none taken from the code under test.  Sums and f32 gradients: 1e-5 rel-L2, the project's tolerance of an fp32 operation
(BASELINE.md §3); a bf16 gradient: 2^-8 rel-L2, one bf16 rounding per element, the restatement evaluated on the bf16-rounded
input.  The cancelling case (physical statistics, |residual| about 1 % of the geopotential term): the kernel's distance from fp64
is at most 2 x that of the reference's formula in plain fp32 torch on the same input (the factor allows for another summation
order over the plane); both distances are printed.  The mean of the preparation pass: E 2^-24 mean_e |x_e| per element, the
bound of a recursive fp32 sum (a bf16 output adds its own rounding, 2^-8 |mean|); its f32 tendencies are bit-equal to torch.
Handler: per-loss vectors 1e-5, scalar and gradient 1e-4 (the project's fp32 end-to-end tolerance)."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _losshandler_ref as ref          # noqa: E402
from conftest import load_golden, rel_l2          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("losshandler.npz")
CASES = ("l2_eval", "multistep", "mixed_dry", "mixed_moist", "balanced", "running_stats")
LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 800, 850, 900, 925, 950, 1000]
F32, BF16 = torch.float32, torch.bfloat16
U24 = 2.0 ** -24


def _t(key):
    return torch.from_numpy(G[key])


def _meta(name):
    return json.loads(str(G[f"{name}/meta"]))


def names_of(K):
    """K levels of z, t and q, not in pressure order, between surface channels"""
    lv = LEVELS[-K:]
    order = [lv[(5 * i + 3) % K] for i in range(K)] if K % 5 else lv[::-1]
    assert sorted(order) == lv
    return ["u10m"] + [f"{v}{p}" for p in order for v in ("t", "z", "q")] + ["sp"]


def stats_of(names):
    """normalisation statistics of realistic size per channel name: (1, C, 1, 1) bias and scale, fp32"""
    bias, scale = [], []
    for n in names:
        if n in ("u10m", "sp"):
            b, s = {"u10m": (0.5, 5.0), "sp": (9.7e4, 9.0e3)}[n]
        else:
            k = math.log(1000.0 / int(n[1:])) / math.log(20.0)
            b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3 * (0.8 + 0.4 * k)), "t": (285.0 - 70.0 * k, 15.0 - 6.0 * k),
                    "q": (2.0e-3 * (1.0 - k) ** 3 + 2e-6, 2.0e-3 * (1.0 - k) ** 3 + 1e-6)}[n[0]]
        bias.append(b)
        scale.append(s)
    return torch.tensor(bias, dtype=F32).view(1, -1, 1, 1), torch.tensor(scale, dtype=F32).view(1, -1, 1, 1)


def hydro_module(K, shape, moist, **kw):
    import makani_amd as ma
    names = names_of(K)
    bias, scale = stats_of(names)
    return ma.HydrostaticBalanceLoss(shape, shape, (0, 0), names, "equiangular", bias, scale, p_min=0, p_max=1000,
                                     use_moist_air_formula=moist, **kw).to(DEV)


def on_gpu(x, dtype, offset=False):
    """x on the GPU in ``dtype``; ``offset``: a contiguous view that starts one element behind an aligned base"""
    x = x.to(dtype)
    if not offset:
        return x.to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
    buf[1:] = x.flatten().to(DEV)
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 != 0
    return v


def hydro_run(K, shape, dtype, moist, wgt, steps=1, offset=False, B=2, seed=0):
    """(sums, gradient) of the kernels and of the restatement on the same input, upstream gradient and weight"""
    from makani_amd import ops
    gen = torch.Generator().manual_seed(1000 * K + shape[0] + seed)
    m = hydro_module(K, shape, moist)
    C, H, W = len(m.channel_names), *shape
    x = on_gpu(torch.randn(B, steps * C, H, W, generator=gen), dtype, offset).detach().requires_grad_(True)
    g = torch.randn(B, steps * (K - 1), generator=gen)
    w = {None: None, "sample": torch.rand(B, 1, H, W, generator=gen) + 0.5, "level": torch.rand(1, K - 1, H, W, generator=gen) + 0.5}[wgt]
    if w is not None and steps > 1 and wgt == "level":
        w = w.repeat(1, steps, 1, 1)
    q = m.quadrature.quad_weight
    sums = ops.HydroSumsFn.apply(x, w.to(DEV) if w is not None else None, q.reshape(-1), m._tables(x.device), steps)
    (gx,) = torch.autograd.grad(sums, x, g.to(DEV))
    assert sums.dtype == F32 and tuple(sums.shape) == (B, steps * (K - 1)) and gx.dtype == dtype and gx.shape == x.shape
    N = B * steps
    x64 = x.detach().cpu().double().reshape(N, C, H, W)
    w64 = None if w is None else w.double().expand(B, steps * (K - 1), H, W).reshape(N, K - 1, H, W)
    args = (m.bias.cpu(), m.scale.cpu(), m.cmat.cpu(), m.z_idx, m.t_idx, m.q_idx if moist else None, q.cpu().double()[0, 0])
    want = ref.hydro_sums(x64, *args, wgt=w64).reshape(B, -1)
    gwant = ref.hydro_grad(x64, *args, g.reshape(N, K - 1), wgt=w64).reshape(x.shape)
    return sums, gx, want, gwant


def check_hydro(dtype, sums, gx, want, gwant, what):
    es, eg = rel_l2(sums, want), rel_l2(gx, gwant)
    print(f"{what}: sums {es:.2e} grad {eg:.2e}")
    assert es <= 1e-5, (what, es)
    assert eg <= (1e-5 if dtype == F32 else 2.0 ** -8), (what, eg)


@pytest.mark.parametrize("K", [2, 3, 13, 16])
@pytest.mark.parametrize("wgt", [None, "sample", "level"])
@pytest.mark.parametrize("moist", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_hydro_kernels_against_fp64(dtype, moist, wgt, K):
    check_hydro(dtype, *hydro_run(K, (9, 16), dtype, moist, wgt), f"K={K} {dtype} moist={moist} wgt={wgt}")


@pytest.mark.parametrize("shape,K,offset", [((17, 33), 13, False), ((17, 33), 13, True), ((33, 64), 13, False), ((33, 64), 3, True),
                                            ((181, 364), 3, False)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_hydro_kernels_over_planes(dtype, shape, K, offset):
    """less than a chunk is test_hydro_kernels_against_fp64's 9 x 16; here an odd plane (one point per thread), three chunks with a
    partial last one, more than 64 chunks' worth of points, and views whose base is not 16-byte aligned"""
    from makani_amd._lib import lib
    assert lib().mk_hydro_chunks(33 * 64) == 3 and lib().mk_hydro_chunks(181 * 364) == 64 and lib().mk_hydro_chunks(9 * 16) == 1
    B = 1 if shape[0] > 100 else 2
    check_hydro(dtype, *hydro_run(K, shape, dtype, True, "level", offset=offset, B=B), f"{shape} K={K} {dtype} offset={offset}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("wgt", [None, "sample", "level"])
def test_hydro_steps_are_scored_as_samples(dtype, wgt):
    check_hydro(dtype, *hydro_run(3, (17, 33), dtype, True, wgt, steps=2), f"S=2 {dtype} wgt={wgt}")


def test_hydro_module_returns_the_dtype_of_the_prediction_and_repeats_bit_identically():
    for dtype in (F32, BF16):
        m = hydro_module(13, (33, 64), True)
        x = torch.randn(2, len(m.channel_names), 33, 64, generator=torch.Generator().manual_seed(3)).to(DEV, dtype).requires_grad_(True)
        runs = []
        for _ in range(2):
            out = m(x, None)
            (gx,) = torch.autograd.grad(out.float().sum(), x)
            runs.append((out.detach().clone(), gx.clone()))
        assert runs[0][0].dtype == dtype and tuple(runs[0][0].shape) == (2, 12)
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        rest = [c for c in range(len(m.channel_names)) if c not in m.z_idx + m.t_idx + m.q_idx]
        assert rest and bool((runs[0][1][:, rest] == 0).all())


@pytest.mark.parametrize("moist", [False, True])
def test_hydro_cancelling_case_is_no_further_from_fp64_than_the_fp32_formula(moist):
    """physical statistics (mean geopotentials in balance with the mean temperatures) and columns in near balance: Z_{k+1} = Z_k -
    hl_k (Tv_k + Tv_{k+1}) (1 + 0.01 n) R_d, so the residual is about 1 % of the geopotential term it is the difference of"""
    from makani_amd import ops
    import makani_amd as ma
    K, shape, B = 13, (33, 64), 2
    gen = torch.Generator().manual_seed(77)
    names = names_of(K)
    b32, s32 = stats_of(names)
    m = hydro_module(K, shape, moist)          # (for the level order and the coefficients: they do not depend on the statistics)
    C, q_idx = len(names), ref.levels(names, "q", "t", 0, 1000)[0]
    cm = m.cmat.cpu().double()
    pf = cm[0, m.z_idx[1]]
    # physical statistics: the mean geopotentials are in balance with the mean (virtual) temperatures
    bias = b32.double().reshape(-1)
    tvb = bias[m.t_idx] * (1.0 + ref.Q_MOIST * bias[q_idx]) if moist else bias[m.t_idx]
    for k in range(K - 1):
        bias[m.z_idx[k + 1]] = bias[m.z_idx[k]] - cm[k, m.t_idx[k]] * (tvb[k] + tvb[k + 1]) / pf
    b32 = bias.float().view(1, C, 1, 1)
    m = ma.HydrostaticBalanceLoss(shape, shape, (0, 0), names, "equiangular", b32, s32, p_min=0, p_max=1000, use_moist_air_formula=moist).to(DEV)
    bias, scale = b32.double().reshape(-1), s32.double().reshape(-1)
    phys = bias.view(1, C, 1, 1) + scale.view(1, C, 1, 1) * 0.5 * torch.randn(B, C, *shape, generator=gen, dtype=torch.float64)
    phys[:, q_idx] = bias[q_idx].view(1, K, 1, 1) + scale[q_idx].view(1, K, 1, 1) * 0.5 * torch.rand(B, K, *shape, generator=gen, dtype=torch.float64)
    tv = phys[:, m.t_idx] * (1.0 + ref.Q_MOIST * phys[:, q_idx]) if moist else phys[:, m.t_idx]
    for k in range(K - 1):
        hl = cm[k, m.t_idx[k]]
        noise = 1.0 + 0.01 * torch.randn(B, *shape, generator=gen, dtype=torch.float64)
        phys[:, m.z_idx[k + 1]] = phys[:, m.z_idx[k]] - hl * (tv[:, k] + tv[:, k + 1]) * noise / pf
    x = ((phys - bias.view(1, C, 1, 1)) / scale.view(1, C, 1, 1)).float()
    q = m.quadrature.quad_weight
    args = (m.bias.cpu(), m.scale.cpu(), m.cmat.cpu(), m.z_idx, m.t_idx, q_idx if moist else None, q.cpu().double()[0, 0])
    r = ref.hydro_residuals(x.double(), *args[:-1])
    zterm = pf * (phys[:, m.z_idx[1:]] - phys[:, m.z_idx[:-1]])
    ratio = (r.norm() / zterm.norm()).item()
    assert 0.003 <= ratio <= 0.03, ratio
    want = ref.hydro_sums(x.double(), *args)
    d_torch = rel_l2(ref.hydro_sums_fp32(x, *args[:-1], q.cpu()[0, 0]), want)
    got = ops.HydroSumsFn.apply(x.to(DEV), None, q.reshape(-1), m._tables(torch.device(DEV, 0)), 1)
    d_kernel = rel_l2(got, want)
    print(f"cancelling moist={moist}: |r| / |z term| {ratio:.3e}  kernel {d_kernel:.3e}  fp32 torch formula {d_torch:.3e}")
    assert d_kernel <= 2.0 * d_torch, (d_kernel, d_torch)


def test_hydro_limits_and_cpu_tensors():
    import makani_amd as ma
    from makani_amd import ops
    lv = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 800, 850, 900, 925, 950, 975, 1000]
    names = [f"{v}{p}" for p in lv for v in ("z", "t")]
    with pytest.raises(ValueError, match="at most 16 levels"):
        ma.HydrostaticBalanceLoss((9, 16), (9, 16), (0, 0), names, "equiangular", torch.zeros(1, 34, 1, 1), torch.ones(1, 34, 1, 1))
    with pytest.raises(ValueError, match="2 .. 16 levels"):
        ops.hydro_table(list(range(17)), list(range(17, 34)), [], 34, torch.zeros(34), torch.ones(34), torch.ones(16), 1.0, 0.0, DEV)
    m = hydro_module(3, (9, 16), False)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(2, len(m.channel_names), 9, 16), None)
    with pytest.raises(ValueError, match="expects"):
        m(torch.zeros(2, len(m.channel_names) + 1, 9, 16, device=DEV), None)


# ---- the preparation pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 3, 32])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_loss_prep_every_flag_combination(dtype, E):
    from makani_amd import ops
    gen = torch.Generator().manual_seed(40 + E)
    B, C = 2, 3
    out_round = 0.0 if dtype == F32 else 2.0 ** -8          # the rounding of a bf16 output: 8 significant bits
    for H, W in ((5, 8), (5, 7)):          # C H W a multiple of 4 (16-byte accesses) and odd (one point per thread)
        prd = torch.randn(B, E, C, H, W, generator=gen).to(DEV, dtype)
        tar = torch.randn(B, C, H, W, generator=gen).to(DEV, dtype)
        hist = torch.randn(B, 2 * C, H, W, generator=gen).to(DEV, dtype)
        inp = hist[:, -C:]          # the last step of a flattened history: a view
        inv = 1.0 / E
        p64, t64, i64 = prd.double(), tar.double(), inp.double()
        mean64 = p64.mean(dim=1)
        bound = E * U24 * p64.abs().mean(dim=1)
        ups = {k: torch.randn(s, generator=gen).to(DEV, dtype) for k, s in (("mean", (B, C, H, W)), ("prd_t", (B, E, C, H, W)), ("mean_t", (B, C, H, W)))}
        for flags in range(1, 16):
            x = prd.detach().requires_grad_(True)
            mean, prd_t, mean_t, tar_t = ops.LossPrepFn.apply(x, tar, inp, flags, inv)
            sel = [bool(flags & f) for f in (ops.PREP_MEAN, ops.PREP_MEMBER_T, ops.PREP_MEAN_T, ops.PREP_TAR_T)]
            assert [o is not None for o in (mean, prd_t, mean_t, tar_t)] == sel, flags
            if mean is not None:
                assert mean.dtype == dtype
                assert bool(((mean.double() - mean64).abs() <= bound + out_round * mean64.abs()).all()), (flags, "mean")
                if E == 1:
                    assert torch.equal(mean, prd[:, 0])
            if prd_t is not None:          # one subtraction: the bits of torch's
                assert torch.equal(prd_t, prd - inp.unsqueeze(1)), (flags, "prd_t")
            if tar_t is not None:
                assert torch.equal(tar_t, tar - inp) and not tar_t.requires_grad, (flags, "tar_t")
            if mean_t is not None:
                w64 = mean64 - i64
                assert bool(((mean_t.double() - w64).abs() <= bound + (U24 + out_round) * w64.abs()).all()), (flags, "mean_t")
                if E == 1:
                    assert torch.equal(mean_t, prd[:, 0] - inp)
            # backward: g_prd = g_prd_t + inv (g_mean + g_mean_t), absent terms skipped
            outs = [(o, ups[k]) for o, k in ((mean, "mean"), (prd_t, "prd_t"), (mean_t, "mean_t")) if o is not None]
            if not outs:
                continue
            (gx,) = torch.autograd.grad([o for o, _ in outs], x, [u for _, u in outs])
            g_mean = ups["mean"] if mean is not None else None
            g_mean_t = ups["mean_t"] if mean_t is not None else None
            g_prd_t = ups["prd_t"] if prd_t is not None else None
            want = ref.prep_bwd(E, inv, g_prd_t, g_mean, g_mean_t)
            mag = torch.zeros_like(p64)          # the magnitudes that are added: three fp32 roundings at the most
            if g_prd_t is not None:
                mag = mag + g_prd_t.double().abs()
            for g in (g_mean, g_mean_t):
                if g is not None:
                    mag = mag + (g.double().abs() * inv).unsqueeze(1)
            assert gx.dtype == dtype and bool(((gx.double() - want).abs() <= 4 * U24 * mag + out_round * want.abs()).all()), (flags, "backward")


def test_loss_prep_limits():
    from makani_amd import ops
    with pytest.raises(NotImplementedError, match="at most 32 members"):
        ops.LossPrepFn.apply(torch.zeros(1, 33, 1, 2, 2, device=DEV), None, None, ops.PREP_MEAN, 1 / 33)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.LossPrepFn.apply(torch.zeros(1, 2, 1, 2, 2), None, None, ops.PREP_MEAN, 0.5)


# ---- drift regularization ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 2])
def test_drift_regularization_against_fp64(p):
    import makani_amd as ma
    gen = torch.Generator().manual_seed(9)
    names = ["a", "b", "c"]
    m = ma.DriftRegularization((17, 33), (17, 33), (0, 0), names, p=p).to(DEV)
    assert m.type == "probabilistic" and m.n_channels == 3
    quad = ref.quad_weights(17, 33)
    assert rel_l2(m.quadrature.quad_weight[0, 0], quad) <= 1e-6
    tar = torch.randn(2, 3, 17, 33, generator=gen) + 0.3
    for shape in ((2, 3, 17, 33), (2, 4, 3, 17, 33)):
        prd = (torch.randn(shape, generator=gen) + 0.1).to(DEV).requires_grad_(True)
        out = m(prd, tar.to(DEV))
        g = torch.randn(2, 3, generator=gen)
        (gx,) = torch.autograd.grad(out, prd, g.to(DEV))
        p64 = prd.detach().cpu().double().requires_grad_(True)
        want = ref.drift(p64, tar, m.quadrature.quad_weight.cpu().double()[0, 0], p)
        (gw,) = torch.autograd.grad(want, p64, g.double())
        assert tuple(out.shape) == (2, 3)
        assert rel_l2(out, want) <= 1e-5 and rel_l2(gx, gw) <= 1e-5, (shape, rel_l2(out, want), rel_l2(gx, gw))


# ---- LossHandler against the recorded reference -----------------------------------------------------------------------------
def _handler(name, **kw):
    import makani_amd as ma
    meta = _meta(name)
    h = ma.LossHandler(ref.params_of(meta), bias=_t("bias"), scale=_t("scale"), time_diff_stds=_t("time_diff_stds"), **meta["handler_kwargs"], **kw)
    return h.train(meta["training"]).to(DEV)


def _inputs(name, call="R"):
    return [t.to(DEV) if t is not None else None for t in ref.case_inputs(G, name, call)]


@pytest.mark.parametrize("name", CASES)
def test_handler_reproduces_the_recorded_reference(name):
    h = _handler(name)
    meta = _meta(name)
    if name == "running_stats":
        prd, tar, inp = _inputs(name, 0)
        h(prd, tar, None, inp)
    else:          # the reference's state in front of the recorded call (balanced: after 101 updates), loaded strictly
        h.load_state_dict({k: _t(f"{name}/before/{k}") for k in meta["persistent"]}, strict=True)
    vectors = []
    hooks = [fn.register_forward_hook(lambda m, i, o: vectors.append(o.detach().clone())) for fn in h.loss_fn]
    prd, tar, inp = _inputs(name)
    prd.requires_grad_(True)
    loss = h(prd, tar, None, inp)
    (grad,) = torch.autograd.grad(loss, prd)
    for k in hooks:
        k.remove()
    errs = {f"vec{i}": rel_l2(v, _t(f"{name}/vec{i}")) for i, v in enumerate(vectors)}
    assert len(vectors) == len(meta["losses"])
    e_loss = abs(loss.item() - float(G[f"{name}/loss"])) / abs(float(G[f"{name}/loss"]))
    e_grad = rel_l2(grad, _t(f"{name}/grad"))
    e_buf = {k: rel_l2(getattr(h, k), _t(f"{name}/buf/{k}")) for k in ("running_mean", "running_var")}
    print(name, " ".join(f"{k} {v:.1e}" for k, v in errs.items()), f"loss {e_loss:.1e} grad {e_grad:.1e}", e_buf)
    assert max(errs.values()) <= 1e-5, errs
    assert e_loss <= 1e-4 and e_grad <= 1e-4, (e_loss, e_grad)
    assert max(e_buf.values()) <= 1e-5 and torch.equal(h.num_batches_tracked.cpu(), _t(f"{name}/buf/num_batches_tracked")), e_buf


def test_handler_forward_and_backward_replay_from_a_captured_graph():
    h = _handler("mixed_moist")
    prd, tar, inp = _inputs("mixed_moist")
    prd.requires_grad_(True)

    def step():
        loss = h(prd, tar, None, inp)
        (g,) = torch.autograd.grad(loss, prd)
        return loss, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager_loss, eager_grad = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_loss, eager_grad = eager_loss.clone(), eager_grad.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss) and torch.equal(grad, eager_grad)


def test_handler_refusals():
    import makani_amd as ma
    meta = _meta("l2_eval")
    p = ref.params_of(meta)
    p.random_slice_loss = True
    with pytest.raises(NotImplementedError, match="random_slice_loss"):
        ma.LossHandler(p)
    h = _handler("mixed_dry")
    prd, tar, inp = _inputs("mixed_dry")
    with pytest.raises(ValueError, match="Channel mismatch: prediction has 11 channels but input has 10 channels"):
        h(prd, tar, None, inp[:, :20])
    with pytest.raises(RuntimeError, match="GPU"):
        h(prd.cpu(), tar.cpu(), None, inp.cpu())
