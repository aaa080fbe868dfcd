"""SpectralAMSELoss, EnsembleNLLLoss and GaussianMMDLoss on the GPU (csrc/amse.hip, csrc/ensnll.hip, csrc/escore.hip) against
the fp64 restatement of tests/_restloss_ref.py, at the shapes of tests/test_gpu_escore.py: a 91 x 180 grid (16 380 points: not
a multiple of the block, several chunks), B = 2, C = 3, E = 1, 2, 5, 9, 32 for the ensemble losses, bf16 members once.  AMSE
takes no lmax (its transform runs at the grid's bandlimit, as the reference's), so lmax = mmax = 46 is the legendre-gauss grid
47 x 92 (a per-degree row shorter than a wave); the 91 x 180 legendre-gauss grid adds rows of 90 orders (a wave and a tail).
Value and gradient (AMSE: target gradient too) <= 1e-5 relative L2 (fp32); a second pass on the same inputs
is bit-identical.

The inputs are conditioned so that 1e-5 tests the kernels and not cancellation, and the reference FORMULA in plain fp32 torch
on the CPU meets the same 1e-5 against the restatement on them (test_inputs_let_the_fp32_formula_meet_the_tolerance asserts
it, no GPU needed):
  * AMSE: prediction and target share one part and carry independent parts of the same power, each white noise plus a smooth
    large-scale field (the white part alone leaves the low degrees almost empty: tests/test_gpu_escore.py).  Coherence about
    1/2; the low degrees hold a handful of coefficients and scatter around it: |coherence| < 0.97 is asserted for every degree
    >= 1, so 1 - coh >= 0.03 carries a relative rounding error below 2^-24 / 0.03 = 2e-6.  Degree 0 holds ONE real
    coefficient: its coherence is +-1 whatever the fields are.
  * NLL: members = a common field (std 3) + the offsets e - (E - 1) / 2 + BOUNDED noise (uniform, |.| <= 0.35): two members
    are never closer than 0.3, the variance is >= 0.0225 everywhere for E >= 2 (eps^2 = 1e-12; asserted > 1e-2), no point sits
    at the clamp; E = 1 sits at it everywhere.
  * MMD: member noise of std 2 plus offsets 0.05 e, so that the distances of all pairs stay within a factor 3 of each other;
    sigma = 80 (beta = 2, per channel) and 20 (beta = 1, channels summed): every exponent d^2 / 2 sigma of every case lies in
    [0.05, 4] (asserted on the restatement).
fp32 torch formula against the restatement on these inputs, worst case over the cases of a loss (value / gradient):
  AMSE 1.1e-07 / 3.8e-07 (target gradient 4.9e-07),  NLL 7.8e-08 / 4.5e-07,  MMD 2.1e-07 / 2.9e-07."""
import math

import pytest
import torch
import torch.nn.functional as F

import _restloss_ref as ref
from _ranks import launch, ranks
from conftest import load_golden, rel_l2

IMG, NAMES = (91, 180), ["u500", "v500", "t2m"]
B, C = 2, len(NAMES)
ES = [1, 2, 5, 9, 32]
TOL = 1e-5
KW = dict(img_shape=IMG, crop_shape=IMG, crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")
AMSE_GRIDS = [(47, 92), (91, 180)]          # legendre-gauss: bandlimit nlat - 1 = 46 (a row shorter than a wave) and 90 (a wave and a tail)
MMD_FORMS = [dict(sigma=80.0), dict(sigma=20.0, alpha=0.9, beta=1.0, channel_reduction=True)]


def _smooth(n, gen, img=IMG):
    s = F.interpolate(torch.randn(n, 1, 4, 8, generator=gen), size=img, mode="bilinear", align_corners=True)
    return s.reshape(n, *img)


def ensemble_inputs(E, seed, offset, cout=C):
    """members of a trained ensemble are close: a common field plus a small member part.  offset 0.05 (MMD): Gaussian member
    noise of std 2 plus a smooth field; offset 1 (NLL): BOUNDED member noise (uniform, |.| <= 0.35) around the offsets e, so
    that two members are never closer than 0.3 and the variance never below 0.0225"""
    gen = torch.Generator().manual_seed(seed)
    if offset == 1.0:
        base = 3.0 * torch.randn(B, C, *IMG, generator=gen)
        o = base + torch.randn(B, C, *IMG, generator=gen)
        f = (base.unsqueeze(1) + 0.7 * (torch.rand(B, E, C, *IMG, generator=gen) - 0.5)
             + (torch.arange(E) - 0.5 * (E - 1)).reshape(1, E, 1, 1, 1))
    else:
        o = 10.0 * torch.randn(B, C, *IMG, generator=gen)
        f = (o.unsqueeze(1) + 2.0 * torch.randn(B, E, C, *IMG, generator=gen) + 2.0 * _smooth(B * E * C, gen).reshape(B, E, C, *IMG)
             + offset * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1))
    w = torch.rand(B, C, *IMG, generator=gen) + 0.5
    g_out = torch.randn(B, cout, generator=gen)
    return f, o, w, g_out


def amse_inputs(grid):
    img = AMSE_GRIDS[grid]
    gen = torch.Generator().manual_seed(7 + grid)

    def part():
        return torch.randn(B, C, *img, generator=gen) + _smooth(B * C, gen, img).reshape(B, C, *img)

    common = part()
    prd, tar = common + part(), common + part()
    w = torch.rand(1, C, img[0] - 1, 1, generator=gen) + 0.5
    g_out = torch.randn(B, C, generator=gen)
    return prd, tar, w, g_out


_REF = {}


def restatement(key):
    """(value, gradient(s), extras) of the fp64 restatement for a case, computed once per process"""
    if key in _REF:
        return _REF[key]
    kind = key[0]
    if kind == "amse":
        prd, tar, w, g_out = amse_inputs(key[2])
        p, t = prd.double().requires_grad_(True), tar.double().requires_grad_(True)
        val, coh = ref.amse(p, t, AMSE_GRIDS[key[2]], "legendre-gauss", w if key[1] else None)
        grads = torch.autograd.grad((val * g_out.double()).sum(), (p, t))
        _REF[key] = (val.detach(), grads, coh.detach())
    elif kind == "nll":
        E, dt = key[1], key[2]
        f, o, w, g_out = ensemble_inputs(E, 10 + E, 1.0)
        fr = f.to(dt).double().requires_grad_(True)
        val = ref.ensemble_nll(fr, o, ref.quadrature_weights(IMG), w)
        grads = torch.autograd.grad((val * g_out.double()).sum(), fr)
        _REF[key] = (val.detach(), grads, None)
    else:
        form, E = key[1], key[2]
        kw = MMD_FORMS[form]
        f, o, w, g_out = ensemble_inputs(E, 100 * form + 50 + E, 0.05, 1 if kw.get("channel_reduction") else C)
        if key[3]:          # 5 % NaN observations and one NaN member value
            gen = torch.Generator().manual_seed(3)
            o = torch.where(torch.rand(o.shape, generator=gen) < 0.05, float("nan"), o)
            f[1, E // 2, 1, 40, 77] = float("nan")
        fr = f.double().requires_grad_(True)
        val, expo = ref.gaussian_mmd(fr, o, ref.quadrature_weights(IMG), w, **kw)
        grads = torch.autograd.grad((val * g_out.double()).sum(), fr)
        expo = torch.cat([e.reshape(-1) for e in expo])
        _REF[key] = (val.detach(), grads, (float(expo.min()), float(expo.max())))
    return _REF[key]


CASES = ([("amse", False, 0), ("amse", True, 0), ("amse", True, 1)] + [("nll", E, torch.float32) for E in ES] + [("nll", 5, torch.bfloat16)]
         + [("mmd", form, E, False) for form in range(len(MMD_FORMS)) for E in ES] + [("mmd", 0, 5, True)])


def _id(key):
    return "-".join(str(k).replace("torch.", "") for k in key)


def _fp32_formula(key):
    """the reference's formula in plain fp32 torch on the CPU: (value, gradients)"""
    kind = key[0]
    if kind == "amse":
        from oracle import sht as osht
        prd, tar, w, g_out = amse_inputs(key[2])
        p, t = prd.clone().requires_grad_(True), tar.clone().requires_grad_(True)
        img = AMSE_GRIDS[key[2]]
        sht = osht.RealSHT(*img, lmax=img[0] - 1, mmax=img[0] - 1, grid="legendre-gauss")
        x, y = sht(p), sht(t)
        xx, yy, xy = torch.square(torch.abs(x)), torch.square(torch.abs(y)), torch.real(x * y.conj())
        if key[1]:
            xx, yy, xy = xx * w, yy * w, xy * w
        inv = 1.0 / (4.0 * math.pi)
        xn2, yn2, xys = (inv * (v[..., 0] + 2 * torch.sum(v[..., 1:], dim=-1)) for v in (xx, yy, xy))
        coh = xys / torch.sqrt(xn2 * yn2 + 1e-6)
        val = (torch.square(torch.sqrt(xn2) - torch.sqrt(yn2)) + 2 * torch.maximum(xn2, yn2) * (1 - coh)).sum(-1)
        return val.detach(), torch.autograd.grad((val * g_out).sum(), (p, t))
    q = ref.quadrature_weights(IMG).float()
    if kind == "nll":
        E, dt = key[1], key[2]
        f, o, w, g_out = ensemble_inputs(E, 10 + E, 1.0)
        fr = f.to(dt).float().requires_grad_(True)
        s2, mu = torch.var_mean(fr, dim=1, correction=0)
        s2 = torch.clamp(s2, min=1e-6 ** 2)
        val = torch.sum(0.5 * (torch.log(s2) + torch.square(o - mu) / s2) * q * w, dim=(-2, -1))
        return val.detach(), torch.autograd.grad((val * g_out).sum(), fr)
    form, E = key[1], key[2]
    kw = MMD_FORMS[form]
    beta, sigma, alpha, cr = kw.get("beta", 2.0), kw["sigma"], kw.get("alpha", 1.0), kw.get("channel_reduction", False)
    f, o, w, g_out = ensemble_inputs(E, 100 * form + 50 + E, 0.05, 1 if cr else C)
    fr = f.clone().requires_grad_(True)

    def kern(a, b):
        d = torch.sum((a - b).abs().pow(beta) * q * w, dim=(-2, -1))
        d = d.sum(dim=1, keepdim=True) if cr else d
        return torch.exp(-0.5 * torch.square(d) / sigma)

    skill = sum(kern(o, fr[:, e]) for e in range(E)) / float(E)
    spread = sum((2.0 * kern(fr[:, i], fr[:, j]) for i in range(E) for j in range(i + 1, E)), torch.zeros_like(skill))
    if E > 1:
        spread = spread * (float(E) - 1.0 + alpha) / float(E * E * (E - 1))
    val = skill - 0.5 * spread
    return val.detach(), torch.autograd.grad((val * g_out).sum(), fr)


@pytest.mark.parametrize("key", [k for k in CASES if not (k[0] == "mmd" and k[3])], ids=_id)
def test_inputs_let_the_fp32_formula_meet_the_tolerance(key):
    """the conditioning of the inputs (module docstring), checked without the kernels"""
    want, gw, extra = restatement(key)
    val, grads = _fp32_formula(key)
    errs = [rel_l2(val, want)] + [rel_l2(g, h) for g, h in zip(grads, gw)]
    print(f"{_id(key)}: fp32 torch formula vs fp64 restatement, value / gradients {' '.join(f'{e:.2e}' for e in errs)}")
    assert max(errs) < TOL, errs
    _check_conditioning(key, extra)


def _check_conditioning(key, extra):
    if key[0] == "amse":
        assert float(extra[..., 1:].abs().max()) < 0.97         # (degree 0: one real coefficient, |coherence| = 1 by construction)
    elif key[0] == "nll" and key[1] >= 2:
        f = ensemble_inputs(key[1], 10 + key[1], 1.0)[0].to(key[2]).double()
        assert float(f.var(dim=1, correction=0).min()) > 1e-2          # eps^2 = 1e-12
    elif key[0] == "mmd":
        assert 0.05 <= extra[0] and extra[1] <= 4.0, extra


def _module(key, dev):
    import makani_amd as ma
    if key[0] == "amse":
        img = AMSE_GRIDS[key[2]]
        return ma.SpectralAMSELoss(**dict(KW, img_shape=img, crop_shape=img, grid_type="legendre-gauss")).to(dev)
    if key[0] == "nll":
        return ma.EnsembleNLLLoss(**KW).to(dev)
    return ma.GaussianMMDLoss(**KW, **MMD_FORMS[key[1]]).to(dev)


def _inputs(key, dev):
    """(differentiable inputs, other arguments, g_out) on the device"""
    if key[0] == "amse":
        prd, tar, w, g_out = amse_inputs(key[2])
        return [prd.to(dev), tar.to(dev)], [w.to(dev) if key[1] else None], g_out.to(dev)
    if key[0] == "nll":
        f, o, w, g_out = ensemble_inputs(key[1], 10 + key[1], 1.0)
        return [f.to(key[2]).to(dev)], [o.to(dev), w.to(dev)], g_out.to(dev)
    kw = MMD_FORMS[key[1]]
    f, o, w, g_out = ensemble_inputs(key[2], 100 * key[1] + 50 + key[2], 0.05, 1 if kw.get("channel_reduction") else C)
    if key[3]:
        gen = torch.Generator().manual_seed(3)
        o = torch.where(torch.rand(o.shape, generator=gen) < 0.05, float("nan"), o)
        f[1, key[2] // 2, 1, 40, 77] = float("nan")
    return [f.to(dev)], [o.to(dev), w.to(dev)], g_out.to(dev)


def _run(mod, diff, rest, g_out):
    xs = [x.clone().requires_grad_(True) for x in diff]
    out = mod(*xs, *rest)
    return out, torch.autograd.grad((out.float() * g_out).sum(), xs)


@pytest.mark.gpu
@pytest.mark.parametrize("key", CASES, ids=_id)
def test_matches_fp64_restatement_and_is_deterministic(key):
    dev = "cuda:0"
    mod = _module(key, dev)
    if key[0] == "amse":
        assert mod.sht.lmax == mod.sht.mmax == AMSE_GRIDS[key[2]][0] - 1 and (key[2] != 0 or mod.sht.lmax == 46)
    diff, rest, g_out = _inputs(key, dev)
    out, grads = _run(mod, diff, rest, g_out)
    out2, grads2 = _run(mod, diff, rest, g_out)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    want, gw, extra = restatement(key)
    _check_conditioning(key, extra)
    errs = [rel_l2(out, want)] + [rel_l2(g.float(), h) for g, h in zip(grads, gw)]
    print(f"{_id(key)}: value / gradients {' '.join(f'{e:.2e}' for e in errs)}")
    assert out.shape == want.shape and out.dtype == torch.float32
    assert errs[0] < TOL, errs
    if key[0] == "nll" and key[2] == torch.bfloat16:
        # the same fp32 gradient, rounded once to bf16: relative error per element at most 2^-9 (half a unit of 8 mantissa bits)
        assert grads[0].dtype == torch.bfloat16 and errs[1] < 2.0 ** -9, errs
    else:
        assert max(errs[1:]) < TOL, errs
    if key[0] == "mmd" and key[3]:          # a point without an observation, or with a NaN member, moves nothing
        f, o = diff[0].cpu(), rest[0].cpu()
        masked = (torch.isnan(o) | torch.isnan(f).any(dim=1)).unsqueeze(1).expand_as(f)
        g = grads[0].cpu()
        assert int(masked.sum()) > 0 and bool((g[masked] == 0).all()) and bool(torch.isfinite(g).all())


@pytest.mark.gpu
def test_recorded_reference_cases_on_the_gpu():
    """the 17 x 32 cases recorded from the reference's classes (tests/test_restloss.py pins the restatement to them) through
    the HIP classes; the E = 1 likelihood case sits at the clamp everywhere"""
    import makani_amd as ma
    dev = "cuda:0"
    cases = ref.load_cases(load_golden("rest_losses.npz"))
    assert len(cases) == 10
    for name, c in cases.items():
        mod = getattr(ma, c["cls"])(**c["kwargs"]).to(dev)
        a = c["a"].to(dev).requires_grad_(True)
        out = mod(a, c["b"].to(dev), c["weights"].to(dev) if c["weights"] is not None else None)
        (g,) = torch.autograd.grad(out.sum(), a)
        errs = rel_l2(out, c["out"]), rel_l2(g, c["grad"])
        print(f"{name}: value {errs[0]:.2e} gradient {errs[1]:.2e}")
        assert out.shape == c["out"].shape and max(errs) < TOL, (name, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [("amse", True, 0), ("nll", 5, torch.float32), ("mmd", 0, 5, False)], ids=_id)
def test_forward_and_backward_replay_from_a_captured_graph(key):
    dev = "cuda:0"
    mod = _module(key, dev)
    diff, rest, g_out = _inputs(key, dev)
    _run(mod, diff, rest, g_out)                            # warms up plans outside the capture
    static = [x.clone().requires_grad_(True) for x in diff]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = mod(*static, *rest)
            grads = torch.autograd.grad((out.float() * g_out).sum(), static)
    torch.cuda.current_stream().wait_stream(stream)
    gen = torch.Generator().manual_seed(99)
    for _ in range(2):
        fresh = [x + 0.5 * torch.randn(x.shape, generator=gen).to(x) for x in diff]
        with torch.no_grad():
            for s, x in zip(static, fresh):
                s.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        want, gw = _run(mod, fresh, rest, g_out)
        assert torch.equal(out, want) and all(torch.equal(a, b) for a, b in zip(grads, gw))


# ---- several processes on one GPU ---------------------------------------------------------------------------------------
def _worker_ensemble(rank, world, rendezvous):
    """two ensemble ranks, four members each: NLL and MMD with ensemble_distributed=True against the serial modules on the
    gathered ensemble (value) and its local members (gradient)"""
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        mcomm.init(1, 1, ensemble=2)
        ie = mcomm.get_rank("ensemble")
        assert mcomm.get_size("ensemble") == 2 and ie == rank
        torch.manual_seed(3)
        img, El = (19, 36), 4
        f_all = torch.randn(2, 2 * El, C, *img)
        o, w = torch.randn(2, C, *img).to(dev), (torch.rand(2, C, *img) + 0.5).to(dev)
        kw = dict(KW, img_shape=img, crop_shape=img)
        for cls, extra in [(ma.EnsembleNLLLoss, dict()), (ma.GaussianMMDLoss, dict()),
                           (ma.GaussianMMDLoss, dict(channel_reduction=True, beta=1.0, sigma=8.0))]:
            ser, par = cls(**extra, **kw).to(dev), cls(ensemble_distributed=True, **extra, **kw).to(dev)
            assert par.ensemble_distributed and not ser.ensemble_distributed
            g = torch.randn(2, ser.n_channels, generator=torch.Generator().manual_seed(11)).to(dev)
            fs = f_all.to(dev).requires_grad_(True)
            want = ser(fs, o, w)
            (want * g).sum().backward()
            fl = f_all[:, ie * El:(ie + 1) * El].to(dev).requires_grad_(True)
            out = par(fl, o, w)
            (out * g).sum().backward()
            errs = rel_l2(out, want), rel_l2(fl.grad, fs.grad[:, ie * El:(ie + 1) * El])
            print(f"rank {rank} {cls.__name__} {extra}: value {errs[0]:.2e} gradient {errs[1]:.2e}", flush=True)
            assert max(errs) < TOL, (cls.__name__, errs)


def _worker_spatial(rank, world, rendezvous):
    """h2 x w2: AMSE with spatial_distributed=True on a 37 x 72 grid (19 + 18 latitudes; the w rank 1 holds no order 0)
    against the serial module: value, and the local shards of prediction and target gradient"""
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        _, ih, iw = mcomm.init(2, 2)
        img = (37, 72)
        kw = dict(KW, img_shape=img, crop_shape=img)
        torch.manual_seed(5)
        common = torch.randn(2, C, *img)
        prd, tar = (common + torch.randn(2, C, *img)).to(dev), (common + torch.randn(2, C, *img)).to(dev)
        g = torch.randn(2, C).to(dev)
        ser = ma.SpectralAMSELoss(**kw).to(dev)
        par = ma.SpectralAMSELoss(spatial_distributed=True, **kw).to(dev)
        assert par.spatial_distributed and not ser.spatial_distributed
        L = ser.sht.lmax
        wgt = (torch.rand(1, C, L, L) + 0.5).to(dev)
        sht = par.sht
        assert (sht.m_off != 0) == (iw == 1) and sum(sht.lat_shapes) == 37 and sht.lat_shapes[0] != sht.lat_shapes[1]
        h0, w0 = sum(sht.lat_shapes[:ih]), sum(sht.lon_shapes[:iw])
        hs, ws = slice(h0, h0 + sht.lat_shapes[ih]), slice(w0, w0 + sht.lon_shapes[iw])
        ls = slice(sht.l_off, sht.l_off + sht.l_shapes[ih])
        ms = slice(sht.m_off, sht.m_off + sht.m_shapes[iw])
        for use_w in (False, True):
            ps, ts = prd.clone().requires_grad_(True), tar.clone().requires_grad_(True)
            want = ser(ps, ts, wgt if use_w else None)
            (want * g).sum().backward()
            pl, tl = prd[..., hs, ws].clone().requires_grad_(True), tar[..., hs, ws].clone().requires_grad_(True)
            out = par(pl, tl, wgt[..., ls, ms] if use_w else None)
            (out * g).sum().backward()
            errs = rel_l2(out, want), rel_l2(pl.grad, ps.grad[..., hs, ws]), rel_l2(tl.grad, ts.grad[..., hs, ws])
            print(f"rank {rank} (h {ih}, w {iw}) AMSE weights {use_w}: value {errs[0]:.2e} gradients {errs[1]:.2e} {errs[2]:.2e}", flush=True)
            assert max(errs) < TOL, errs


@pytest.mark.gpu
def test_ensemble_parallel_nll_and_mmd_match_serial():
    launch(_worker_ensemble, 2, limit=240)


@pytest.mark.gpu
def test_spatially_parallel_amse_matches_serial():
    launch(_worker_spatial, 4, limit=240)
