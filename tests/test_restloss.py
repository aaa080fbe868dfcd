"""SpectralAMSELoss, EnsembleNLLLoss and GaussianMMDLoss (csrc/amse.hip, csrc/ensnll.hip, mk_mmd_finish of csrc/escore.hip):
the fp64 restatement of tests/_restloss_ref.py against fixtures recorded in double precision from the reference's own classes
(tools/make_restloss_golden.py), and the constructor / error contract of the three classes on CPU tensors."""
import pytest
import torch

import _restloss_ref as ref
from conftest import load_golden, rel_l2

KW = dict(img_shape=(9, 16), crop_shape=(9, 16), crop_offset=(0, 0), channel_names=["u500", "v500", "t2m"], grid_type="equiangular")
NAMES = ["amse_default", "amse_weights", "nll_single_member_clamped", "nll_three_members", "nll_weights", "mmd_default",
         "mmd_channel_reduction", "mmd_single_member", "mmd_alpha_beta1", "mmd_nan_observations"]
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(ref.load_cases(load_golden("rest_losses.npz")))
    return _CASES


@pytest.mark.parametrize("name", NAMES)
def test_fp64_restatement_matches_the_reference_fixtures(name):
    """value and (autograd) gradient of the test-side formulas against the reference recorded in double precision"""
    c = cases()[name]
    a = c["a"].double().requires_grad_(True)
    q = c["quad_weight"].double() if c["quad_weight"] is not None else None
    out = ref.reference(c["cls"], c["kwargs"], a, c["b"], q, c["weights"])
    (g,) = torch.autograd.grad(out.sum(), a)
    assert out.shape == c["out"].shape and c["out"].dtype == torch.float64
    print(f"{name}: value {rel_l2(out, c['out']):.2e} gradient {rel_l2(g, c['grad']):.2e}")
    assert rel_l2(out, c["out"]) <= 1e-12, (name, rel_l2(out, c["out"]))
    assert rel_l2(g, c["grad"]) <= 1e-12, (name, rel_l2(g, c["grad"]))


def test_the_fixture_covers_what_it_should():
    cs = cases()
    assert sorted(cs) == sorted(NAMES)
    # E = 1: the variance is 0, the clamp is active everywhere; three members of int8 inputs: nowhere
    assert cs["nll_single_member_clamped"]["a"].shape[1] == 1
    f = cs["nll_three_members"]["a"].double()
    assert float(f.var(dim=1, correction=0).min()) > 1e-6
    assert int(torch.isnan(cs["mmd_nan_observations"]["b"]).sum()) > 0
    assert cs["mmd_channel_reduction"]["out"].shape == (2, 1) and cs["mmd_default"]["out"].shape == (2, 3)
    assert cs["mmd_alpha_beta1"]["kwargs"]["alpha"] != 1.0 and cs["mmd_alpha_beta1"]["kwargs"]["beta"] == 1.0
    # the package's quadrature weights are the reference's, bit for bit
    import makani_amd as ma
    m = ma.EnsembleNLLLoss(**cs["nll_weights"]["kwargs"])
    assert torch.equal(m.quad_weight_split.reshape(17, 32), cs["nll_weights"]["quad_weight"])


def test_constructor_contract():
    import makani_amd as ma
    a = ma.SpectralAMSELoss(**KW)
    assert a.type == "deterministic" and a.n_channels == 3 and a.eps == 1.0e-6 and not a.spatial_distributed
    assert a.sht.lmax == 4 and a.lm_weights.shape == (4, 4)
    assert a.compute_channel_weighting("auto").tolist() == pytest.approx([0.5, 0.5, 1.0])
    n = ma.EnsembleNLLLoss(**KW)
    assert n.type == "probabilistic" and n.n_channels == 3 and n.eps == 1.0e-6
    assert not n.ensemble_distributed and not n.spatial_distributed
    assert n.compute_channel_weighting("auto").tolist() == pytest.approx([0.5, 0.5, 1.0])
    m = ma.GaussianMMDLoss(**KW)
    assert (m.sigma, m.alpha, m.beta, m.channel_reduction) == (1.0, 1.0, 2.0, False)
    assert m.type == "probabilistic" and m.n_channels == 3 and ma.GaussianMMDLoss(channel_reduction=True, **KW).n_channels == 1
    assert m.ensemble_weights is None and not m.ensemble_distributed and not m.spatial_distributed
    assert m.compute_channel_weighting("auto", None).tolist() == [1.0]
    for mod in (n, m):
        assert mod.quad_weight_split.shape == (1, 1, 144) and abs(float(mod.quad_weight_split.sum()) - 1.0) < 1e-6
    for mod in (a, n, m):
        assert len(mod.state_dict()) == 0


def test_errors_on_cpu_tensors():
    import makani_amd as ma
    f4, f5, o = torch.zeros(2, 3, 9, 16), torch.zeros(2, 2, 3, 9, 16), torch.zeros(2, 3, 9, 16)
    with pytest.raises(ValueError, match="forecasts tensor expected to have 5 dimensions but found 4"):
        ma.GaussianMMDLoss(**KW)(f4, o)
    with pytest.raises(ValueError, match="expected 5"):                 # the reference unpacks the five axes
        ma.EnsembleNLLLoss(**KW)(f4, o)
    with pytest.raises(ValueError, match=r"the weights have to have the same number of dimensions \(found 2\) as observations \(found 4\)"):
        ma.GaussianMMDLoss(**KW)(f5, o, torch.ones(9, 16))
    with pytest.raises(ValueError, match="the weights have to have the same number of dimensions as observations"):
        ma.EnsembleNLLLoss(**KW)(f5, o, torch.ones(9, 16))
    with pytest.raises(NotImplementedError, match="currently only constant ensemble weights are supported"):
        ma.GaussianMMDLoss(ensemble_weights=torch.ones(2), **KW)(f5, o)
    big = torch.zeros(1, 33, 3, 9, 16)
    for cls in (ma.EnsembleNLLLoss, ma.GaussianMMDLoss):
        with pytest.raises(NotImplementedError, match="ensemble size 33"):
            cls(**KW)(big, o[:1])
        with pytest.raises(RuntimeError, match="GPU"):                  # no CPU fallback
            cls(**KW)(f5, o)
    with pytest.raises(RuntimeError, match="GPU"):
        ma.SpectralAMSELoss(**KW)(f4, o)
    with pytest.raises(NotImplementedError):
        ma.GaussianMMDLoss(beta=0.5, **KW)
