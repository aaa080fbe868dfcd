"""The ensemble energy-score losses (csrc/escore.hip; LpEnergyScoreLoss / L2EnergyScoreLoss, SobolevEnergyScoreLoss,
SpectralL2EnergyScoreLoss) against fixtures recorded from the reference's own ``makani/utils/losses/energy_score.py``
(tools/make_escore_golden.py): constructor contract, value and forecast gradient, the NaN and eps masks, bf16 members, the
ensemble-parallel path.  fp32 tolerance 1e-5."""
import pytest
import torch

import _escore_ref as ref
from _ranks import launch, ranks
from conftest import load_golden, rel_l2

KW = dict(img_shape=(9, 16), crop_shape=(9, 16), crop_offset=(0, 0), channel_names=["u500", "v500", "t2m"], grid_type="equiangular")
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(ref.load_cases(load_golden("escore_losses.npz")))
    return _CASES


def test_escore_constructor_contract():
    import makani_amd as ma
    assert ma.L2EnergyScoreLoss is ma.LpEnergyScoreLoss
    m = ma.LpEnergyScoreLoss(**KW)
    assert (m.p, m.alpha, m.beta, m.eps, m.spread_temper_steps, m.channel_reduction) == (2.0, 1.0, 1.0, 1.0e-6, 0, True)
    assert m.quad_weight_split.shape == (1, 1, 144) and abs(float(m.quad_weight_split.sum()) - 1.0) < 1e-6
    assert m.ensemble_weights is None and not m.ensemble_distributed and not m.spatial_distributed
    s = ma.SobolevEnergyScoreLoss(**KW)
    assert (s.offset, s.fraction, s.relative_weight, s.alpha, s.beta, s.eps) == (1.0, 1.0, 1.0, 1.0, 1.0, 1.0e-6)
    L = s.sht.lmax
    assert L == 4 and s.lm_weights.shape == (L, L)
    l = torch.arange(L, dtype=torch.float32)
    assert torch.allclose(s.lm_weights[:, 0], 1.0 + l * (l + 1)) and torch.allclose(s.lm_weights[:, 1], 2.0 * (1.0 + l * (l + 1)))
    s2 = ma.SobolevEnergyScoreLoss(fraction=0.5, offset=0.5, relative_weight=2.0, **KW)
    assert torch.allclose(s2.lm_weights[:, 2], 2.0 * (0.5 + 2.0 * l * (l + 1)).sqrt())
    t = ma.SpectralL2EnergyScoreLoss(lmax=3, **KW)
    assert t.sht.lmax == 3 and t.lm_weights.shape == (3, 3)
    assert torch.allclose(t.lm_weights[1], torch.tensor([1.0, 2.0, 2.0]) / (4.0 * torch.pi))
    for cls in (ma.LpEnergyScoreLoss, ma.SobolevEnergyScoreLoss, ma.SpectralL2EnergyScoreLoss):
        on, off = cls(**KW), cls(channel_reduction=False, **KW)
        assert on.type == "probabilistic" and (on.n_channels, off.n_channels) == (1, 3)
        assert on.compute_channel_weighting("auto").tolist() == [1.0]
        assert off.compute_channel_weighting("auto").tolist() == pytest.approx([0.5, 0.5, 1.0])
        with pytest.raises(ValueError, match="forecasts tensor expected to have 5 dimensions but found 4"):
            on(torch.zeros(2, 3, 9, 16), torch.zeros(2, 3, 9, 16))
        with pytest.raises(NotImplementedError, match="currently only constant ensemble weights are supported"):
            cls(ensemble_weights=torch.ones(2), **KW)(torch.zeros(2, 2, 3, 9, 16), torch.zeros(2, 3, 9, 16))


def test_escore_p_below_one_raises():
    import makani_amd as ma
    with pytest.raises(NotImplementedError):
        ma.LpEnergyScoreLoss(p=0.5, **KW)
    assert ma.LpEnergyScoreLoss(p=1, **KW).p == 1.0


def test_escore_weights_need_the_dimensions_of_the_observations():
    import makani_amd as ma
    with pytest.raises(ValueError, match="the weights have to have the same number of dimensions"):
        ma.LpEnergyScoreLoss(**KW)(torch.zeros(2, 2, 3, 9, 16), torch.zeros(2, 3, 9, 16), torch.ones(9, 16))


def test_fp64_restatement_matches_the_reference_fixtures():
    """the test-side formulas themselves: value and (autograd) gradient against the recorded reference at 1e-6"""
    for name, c in cases().items():
        f = c["forecasts"].double().requires_grad_(True)
        out = ref.reference(c["cls"], c["kwargs"], f, c["observations"], c["weights"], ref.temper_scale(c))
        (g,) = torch.autograd.grad(out.sum(), f)
        assert out.shape == c["out"].shape, name
        assert rel_l2(out, c["out"]) < 1e-6, (name, rel_l2(out, c["out"]))
        assert rel_l2(g, c["grad"]) < 1e-6, (name, rel_l2(g, c["grad"]))


def _run(c, dev="cuda:0"):
    import makani_amd as ma
    mod = getattr(ma, c["cls"])(**c["kwargs"]).to(dev)
    mod.train(c["train"])
    f = c["forecasts"].to(dev).requires_grad_(True)
    w = c["weights"].to(dev) if c["weights"] is not None else None
    if c["cls"] == "LpEnergyScoreLoss":
        out = mod(f, c["observations"].to(dev), w, lead_time_step=c["lead_time_step"])
    else:
        out = mod(f, c["observations"].to(dev))
    (g,) = torch.autograd.grad(out.sum(), f)
    return out, g


@pytest.mark.gpu
def test_escore_matches_reference_golden():
    assert len(cases()) == 11
    for name, c in cases().items():
        out, g = _run(c)
        assert out.shape == c["out"].shape and out.dtype == torch.float32, name
        print(f"{name}: value {rel_l2(out, c['out']):.2e} gradient {rel_l2(g, c['grad']):.2e}")
        assert rel_l2(out, c["out"]) < 1e-5, (name, rel_l2(out, c["out"]))
        assert rel_l2(g, c["grad"]) < 1e-5, (name, rel_l2(g, c["grad"]))


@pytest.mark.gpu
def test_escore_nan_observations_get_exactly_zero_gradient():
    c = cases()["lp_nan_observations"]
    _, g = _run(c)
    masked = torch.isnan(c["observations"]).unsqueeze(1).expand_as(c["forecasts"])
    assert int(masked.sum()) > 0 and bool((g.cpu()[masked] == 0).all()) and bool(torch.isfinite(g).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["LpEnergyScoreLoss", "SobolevEnergyScoreLoss", "SpectralL2EnergyScoreLoss"])
def test_escore_coincident_members(cls):
    import makani_amd as ma
    torch.manual_seed(5)
    mod = getattr(ma, cls)(**KW).to("cuda:0")
    o = torch.randn(2, 3, 9, 16, device="cuda:0")
    # every member equal to the observation: all sums are below eps, the loss is exactly 0, the gradient finite and 0
    f = o.unsqueeze(1).repeat(1, 3, 1, 1, 1).requires_grad_(True)
    out = mod(f, o)
    (g,) = torch.autograd.grad(out.sum(), f)
    assert bool((out == 0).all()) and bool((g == 0).all())
    # members equal to each other, away from the observation: the skill term of a single member
    one = (o + 1.0 + torch.rand_like(o)).unsqueeze(1)
    f = one.repeat(1, 3, 1, 1, 1).requires_grad_(True)
    out = mod(f, o)
    (g,) = torch.autograd.grad(out.sum(), f)
    single = mod(one, o)
    assert bool(torch.isfinite(g).all()) and rel_l2(out, single) < 1e-6


@pytest.mark.gpu
def test_escore_ensemble_size_limit():
    import makani_amd as ma
    for cls in (ma.LpEnergyScoreLoss, ma.SobolevEnergyScoreLoss, ma.SpectralL2EnergyScoreLoss):
        with pytest.raises(NotImplementedError):
            cls(**KW).to("cuda:0")(torch.zeros(1, 33, 3, 9, 16, device="cuda:0"), torch.zeros(1, 3, 9, 16, device="cuda:0"))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [2.0, 1.0, 1.5])
def test_escore_bf16_forecasts(p):
    import makani_amd as ma
    torch.manual_seed(6)
    mod = ma.LpEnergyScoreLoss(p=p, channel_reduction=False, **KW).to("cuda:0")
    fb = torch.randn(2, 5, 3, 9, 16, device="cuda:0").bfloat16().requires_grad_(True)
    o = torch.randn(2, 3, 9, 16, device="cuda:0")
    ff = fb.detach().float().requires_grad_(True)
    ob, of = mod(fb, o), mod(ff, o)
    (gb,) = torch.autograd.grad(ob.sum(), fb)
    (gf,) = torch.autograd.grad(of.sum(), ff)
    assert gb.dtype == torch.bfloat16 and ob.dtype == torch.float32
    assert rel_l2(ob, of) < 1e-5
    # the same fp32 gradient, rounded once to bf16: relative error per element at most 2^-9 (half a unit of 8 mantissa bits)
    assert rel_l2(gb.float(), gf) < 2.0 ** -9


def _worker_ensemble(rank, world, rendezvous):
    """ensemble_distributed=True (energy_score.py:139-151,188-190,373-386,416-418,559-571,600-602): 2 batch entries x 2 ensemble
    ranks on one GPU, three members per rank: value and local-member gradient of the three classes against the serial modules
    on the gathered ensemble"""
    with ranks(rank, world, rendezvous):
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        mcomm.init(1, 1, ensemble=2)
        ie, ib = mcomm.get_rank("ensemble"), mcomm.get_rank("batch")
        assert (mcomm.get_size("ensemble"), mcomm.get_size("batch"), mcomm.get_size("data")) == (2, 2, 4) and rank == ib * 2 + ie
        torch.manual_seed(3)
        img, C, El = (19, 36), 3, 3
        f_all = torch.randn(2, 2 * El, C, *img)
        o_all = torch.randn(2, C, *img)
        w_all = torch.rand(2, C, *img) + 0.5
        kw = dict(img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_names=[str(k) for k in range(C)], grid_type="equiangular")
        cases = [(ma.LpEnergyScoreLoss, dict(p=1.5, channel_reduction=False), True), (ma.LpEnergyScoreLoss, dict(), False),
                 (ma.SobolevEnergyScoreLoss, dict(), False), (ma.SpectralL2EnergyScoreLoss, dict(channel_reduction=False), False)]
        for cls, extra, use_w in cases:
            ser = cls(**extra, **kw).to(dev)
            par = cls(ensemble_distributed=True, **extra, **kw).to(dev)
            assert par.ensemble_distributed and not ser.ensemble_distributed
            g = torch.randn(2, ser.n_channels, generator=torch.Generator().manual_seed(11))[ib:ib + 1].to(dev)
            fs = f_all[ib:ib + 1].to(dev).requires_grad_(True)
            o = o_all[ib:ib + 1].to(dev)
            args = (w_all[ib:ib + 1].to(dev),) if use_w else ()
            ref_out = ser(fs, o, *args)
            (ref_out * g).sum().backward()
            fl = f_all[ib:ib + 1, ie * El:(ie + 1) * El].to(dev).requires_grad_(True)
            out = par(fl, o, *args)
            (out * g).sum().backward()
            assert rel_l2(out, ref_out) < 1e-5, (cls.__name__, out, ref_out)
            assert rel_l2(fl.grad, fs.grad[:, ie * El:(ie + 1) * El]) < 2e-5, cls.__name__


@pytest.mark.gpu
def test_ensemble_parallel_escore_matches_serial():
    launch(_worker_ensemble, 4, limit=240)
