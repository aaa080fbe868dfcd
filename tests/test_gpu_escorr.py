"""CorrectedSpectralL2EnergyScoreLoss on the row-resident kernels of csrc/escorr.hip against ``restatement`` below, a plain
complex128 restatement of makani/utils/losses/energy_score.py:962-1038 differentiated by autograd (tests/test_escorr.py pins
it to the recorded reference).  1e-5 on value and gradient (fp32); 2e-5 on local gradients under a split.
Kernel level, on coefficients: E = 1, 2 (six sums, 42 slices), 9 (one slice), 32 (three sums per lane); M = 1, 46, and one
below, at and two above the chunk of 128 orders.  Members are a common field (std 10) + 0.3 noise + 0.25 e; the degree l = 3 is
all zeros (the `< eps` branch); NaNs sit in one channel's observation and another's members: they tell a masked P_pred from the
reference's unmasked one (not for E = 1, which has no spread to scale, nor per channel at M = 1, where a NaN masks the degree)."""
import math

import pytest
import torch

import _escore_ref as ref
from _ranks import launch, ranks
from conftest import load_golden, rel_l2

MC = 128          # csrc/escorr.hip: orders per chunk
EPS = 1.0e-6


def restatement(f, o, q, reduce=True, alpha=1.0, beta=1.0, eps=EPS, masked_power=False):
    """f (B, E, C, L, M), o (B, C, L, M) complex128, q (L, M) -> loss (B, C | 1) and every distance sum the eps mask sees.
    masked_power=True is NOT the reference: the spectra under the mask of the distances (the tests show they differ)."""
    E = f.shape[1]
    sq = lambda z: z.real ** 2 + z.imag ** 2
    bad = torch.isnan(o) | torch.isnan(f).any(dim=1)
    fz, oz = torch.where(torch.isnan(f), torch.zeros_like(f), f), torch.where(torch.isnan(o), torch.zeros_like(o), o)
    wq = torch.where(bad, torch.zeros_like(q), q.expand_as(bad))
    pw = wq if masked_power else q.expand_as(bad)
    sums = [(pw.unsqueeze(1) * sq(fz)).sum(-1).mean(1), (pw * sq(oz)).sum(-1),                          # P_pred, P_true (B, C, L)
            (wq.unsqueeze(1) * sq(oz.unsqueeze(1) - fz)).sum(-1),                                       # skill (B, E, C, L)
            (wq[:, None, None] * sq(fz.unsqueeze(1) - fz.unsqueeze(2))).sum(-1)]                        # spread (B, E, E, C, L)
    if reduce:
        sums = [s.sum(dim=-2, keepdim=True) for s in sums]
    ppred, ptrue, skill, spread = sums
    root = lambda v: torch.where(v < eps, torch.zeros_like(v), torch.where(v < eps, torch.ones_like(v), v).pow(beta / 2))
    espread = root(spread).sum(dim=(1, 2)) * ((E - 1 + alpha) / (E * E * (E - 1)) if E > 1 else 0.0)
    loss = root(skill).mean(dim=1) - 0.5 * espread * ptrue / (ppred + eps)
    return loss.sum(dim=-1), torch.cat([skill.reshape(-1), spread.reshape(-1)]).detach()


def module_restatement(kwargs, f, o):
    """the restatement behind the fp64 transform of tests/_escore_ref.py, for a module's constructor kwargs"""
    fc, oc, _, cm, lmax = ref._coefficients(f, o, tuple(kwargs["img_shape"]), kwargs.get("lmax"), kwargs["grid_type"])
    q = (cm / (4 * math.pi))[None, :].expand(lmax, lmax)
    extra = {k: kwargs[k] for k in ("alpha", "beta", "eps") if k in kwargs}
    return restatement(fc, oc, q, kwargs.get("channel_reduction", True), **extra)[0]


def _coefficient_inputs(E, M):
    gen = torch.Generator().manual_seed(100000 + 1000 * E + M)          # (a condition on the inputs is asserted below, in fp64)
    B, C, L = 2, 3, 4
    cn = lambda *shape: torch.complex(torch.randn(*shape, generator=gen, dtype=torch.float64), torch.randn(*shape, generator=gen, dtype=torch.float64))
    common = 10.0 * cn(B, 1, C, L, M)
    f = common + 0.3 * cn(B, E, C, L, M) + 0.25 * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
    o = common[:, 0] + 0.3 * cn(B, C, L, M)
    f[:, :, :, 3], o[:, :, 3] = 0.0, 0.0
    o[:, 1, :3, ::8] = float("nan")
    f[0, E - 1, 0, 1, M // 2] = float("nan")
    f[1, 0, 0, 2, 3 % M::8] = float("nan")
    q = torch.rand(L, M, generator=gen, dtype=torch.float64) + 0.5
    return f.to(torch.complex64), o.to(torch.complex64), q.float()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 46, MC - 1, MC, MC + 2])
@pytest.mark.parametrize("E", [1, 2, 9, 32])
def test_escorr_kernels_match_complex128_restatement(E, M):
    from makani_amd.losses import CorrectedEnergyScoreFn
    dev = "cuda:0"
    f, o, q = _coefficient_inputs(E, M)
    nan_f = torch.isnan(f)
    for reduce in (True, False):
        for beta in (1.0, 0.8):
            g_out = torch.randn(2, 1 if reduce else 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
            fr = f.to(torch.complex128).requires_grad_(True)
            want, sums = restatement(fr, o.to(torch.complex128), q.double(), reduce, 0.9, beta)
            (gw,) = torch.autograd.grad((want * g_out).sum(), fr)
            assert not bool(((sums != 0) & (sums >= EPS / 100) & (sums <= 100 * EPS)).any()), "a sum within a factor 100 of eps"
            assert bool((sums == 0).any())                      # the zero degree: the `< eps` branch runs
            if E > 1 and (M > 1 or reduce):
                masked = restatement(fr.detach(), o.to(torch.complex128), q.double(), reduce, 0.9, beta, masked_power=True)[0]
                assert rel_l2(masked, want) > 1e-3, rel_l2(masked, want)
            runs = []
            for _ in range(2):
                fx = f.to(dev).requires_grad_(True)
                out = CorrectedEnergyScoreFn.apply(fx, o.to(dev), q.to(dev), reduce, beta, 0.9, EPS, [])
                (g,) = torch.autograd.grad((out * g_out.float().to(dev)).sum(), fx)
                runs.append((out.cpu(), g.cpu()))
            (out, g), (out2, g2) = runs
            assert torch.equal(out, out2) and torch.equal(torch.view_as_real(g), torch.view_as_real(g2))
            errs = rel_l2(out, want), rel_l2(torch.view_as_real(g), torch.view_as_real(gw))
            print(f"E={E} M={M} reduce={reduce} beta={beta}: value {errs[0]:.2e} gradient {errs[1]:.2e}")
            assert out.shape == want.shape and max(errs) < 1e-5, errs
            assert bool(torch.isfinite(torch.view_as_real(g)).all()) and bool((g[nan_f] == 0).all())


def _module(kwargs, dev="cuda:0", **extra):
    import makani_amd as ma
    return ma.CorrectedSpectralL2EnergyScoreLoss(**dict(kwargs, **extra)).to(dev)


@pytest.mark.gpu
def test_escorr_module_matches_reference_golden():
    cases = ref.load_cases(load_golden("escorr_losses.npz"))
    assert len(cases) == 4
    for name, c in cases.items():
        f = c["forecasts"].to("cuda:0").requires_grad_(True)
        out = _module(c["kwargs"])(f, c["observations"].to("cuda:0"))
        (g,) = torch.autograd.grad(out.sum(), f)
        errs = rel_l2(out, c["out"]), rel_l2(g, c["grad"])
        print(f"{name}: value {errs[0]:.2e} gradient {errs[1]:.2e}")
        assert out.shape == c["out"].shape and out.dtype == torch.float32 and max(errs) < 1e-5, (name, errs)


def _grid_inputs(img, B, E, C, gen):
    """the input recipe of tests/test_gpu_escore.py (its docstring says why): comparable power at every degree"""
    import torch.nn.functional as F
    o = 10.0 * torch.randn(B, C, *img, generator=gen)
    smooth = F.interpolate(torch.randn(B * E * C, 1, 4, 8, generator=gen), size=img, mode="bilinear", align_corners=True)
    smooth = (smooth - smooth.mean(-1, keepdim=True)).reshape(B, E, C, *img)
    f = o.unsqueeze(1) + 2.0 * torch.randn(B, E, C, *img, generator=gen) + 2.0 * smooth + 0.25 * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
    return f, o


@pytest.mark.gpu
def test_escorr_module_at_91x180_and_from_a_captured_graph():
    img, names, dev = (91, 180), ["u500", "v500", "t2m"], "cuda:0"
    kwargs = dict(img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_names=names, grid_type="legendre-gauss", lmax=46,
                  channel_reduction=False, alpha=0.95)
    gen = torch.Generator().manual_seed(46)
    f, o = _grid_inputs(img, 2, 5, 3, gen)
    g_out = torch.randn(2, 3, generator=gen)
    mod = _module(kwargs)
    fx, od, gd = f.to(dev).requires_grad_(True), o.to(dev), g_out.to(dev)

    def step():
        out = mod(fx, od)
        return out, torch.autograd.grad((out * gd).sum(), fx)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            out, g = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out, g = out.clone(), g.clone()
    fr = f.double().requires_grad_(True)
    want = module_restatement(kwargs, fr, o)
    (gw,) = torch.autograd.grad((want * g_out.double()).sum(), fr)
    errs = rel_l2(out, want), rel_l2(g, gw)
    print(f"91 x 180, E = 5: value {errs[0]:.2e} gradient {errs[1]:.2e}")
    assert out.shape == want.shape and max(errs) < 1e-5, errs
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout, gg = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, out) and torch.equal(gg, g)


def _worker_parallel(rank, world, rendezvous, h, w, ens):
    """2 batch entries x (2 ensemble ranks | h2 | w2) on one GPU: the parallel module against the serial one on the gathered data"""
    with ranks(rank, world, rendezvous):
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        mcomm.init(h, w, ensemble=ens)
        ib, ie, ih, iw = (mcomm.get_rank(k) for k in ("batch", "ensemble", "h", "w"))
        assert mcomm.get_size("batch") == 2
        img, C, El = (37, 72), 3, 4 // ens
        kwargs = dict(img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_names=[str(k) for k in range(C)], grid_type="equiangular",
                      channel_reduction=False, beta=0.8)
        f_all, o_all = _grid_inputs(img, 2, ens * El, C, torch.Generator().manual_seed(3))
        g = torch.randn(2, C, generator=torch.Generator().manual_seed(11))[ib:ib + 1].to(dev)
        ser = _module(kwargs)
        par = _module(kwargs, ensemble_distributed=ens > 1, spatial_distributed=h * w > 1)
        assert par.ensemble_distributed == (ens > 1) and par.spatial_distributed == (h * w > 1)
        hs = ws = slice(None)
        if h * w > 1:
            h0, w0 = sum(par.sht.lat_shapes[:ih]), sum(par.sht.lon_shapes[:iw])
            hs, ws = slice(h0, h0 + par.sht.lat_shapes[ih]), slice(w0, w0 + par.sht.lon_shapes[iw])
        sel = (slice(ib, ib + 1), slice(ie * El, (ie + 1) * El), slice(None), hs, ws)
        fs = f_all[ib:ib + 1].to(dev).requires_grad_(True)
        want = ser(fs, o_all[ib:ib + 1].to(dev))
        (want * g).sum().backward()
        fl = f_all[sel].to(dev).requires_grad_(True)
        out = par(fl, o_all[(sel[0],) + sel[2:]].to(dev).contiguous())
        (out * g).sum().backward()
        errs = rel_l2(out, want), rel_l2(fl.grad, fs.grad[(slice(None),) + sel[1:]])
        print(f"rank {rank} (h {ih}, w {iw}, ensemble {ie}): value {errs[0]:.2e} gradient {errs[1]:.2e}", flush=True)
        assert errs[0] < 1e-5 and errs[1] < 2e-5, errs


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,ens", [(1, 1, 2), (2, 1, 1), (1, 2, 1)])
def test_escorr_parallel_matches_serial(h, w, ens):
    launch(_worker_parallel, 4, h, w, ens, limit=240)
