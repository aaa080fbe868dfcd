"""CorrectedSpectralL2EnergyScoreLoss without a GPU: names, the reference's constructor contract (energy_score.py:859-927), and
the complex128 restatement of tests/test_gpu_escorr.py against the reference's own recorded results (tools/make_escorr_golden.py)."""
import pytest
import torch

import _escore_ref as ref
from conftest import load_golden, rel_l2
from test_gpu_escorr import module_restatement

KW = dict(img_shape=(9, 16), crop_shape=(9, 16), crop_offset=(0, 0), channel_names=["u500", "v500", "t2m"], grid_type="equiangular")


def test_escorr_names_and_constructor_contract():
    import makani_amd as ma
    from makani_amd import losses
    cls = ma.CorrectedSpectralL2EnergyScoreLoss
    assert "CorrectedSpectralL2EnergyScoreLoss" in ma.__all__
    assert not any(getattr(v, "func", v) is cls for v in losses._LOSS_REGISTRY.values())
    on, off = cls(**KW), cls(channel_reduction=False, lmax=3, **KW)
    assert (on.alpha, on.beta, on.eps, on.channel_reduction) == (1.0, 1.0, 1.0e-6, True)
    assert on.ensemble_weights is None and not on.ensemble_distributed and not on.spatial_distributed
    assert on.sht.lmax == 4 and off.sht.lmax == 3 and off.lm_weights.shape == (3, 3)
    assert torch.allclose(off.lm_weights[1], torch.tensor([1.0, 2.0, 2.0]) / (4.0 * torch.pi))
    assert on.type == "probabilistic" and (on.n_channels, off.n_channels) == (1, 3)
    assert on.compute_channel_weighting("auto").tolist() == [1.0]
    assert off.compute_channel_weighting("auto").tolist() == pytest.approx([0.5, 0.5, 1.0])
    with pytest.raises(RuntimeError, match="GPU"):
        on(torch.zeros(2, 2, 3, 9, 16), torch.zeros(2, 3, 9, 16))


def test_escorr_restatement_matches_the_reference_fixtures():
    cases = ref.load_cases(load_golden("escorr_losses.npz"))
    assert sorted(c["forecasts"].shape[1] for c in cases.values()) == [1, 2, 3, 4]
    for name, c in cases.items():
        f = c["forecasts"].double().requires_grad_(True)
        out = module_restatement(c["kwargs"], f, c["observations"])
        (g,) = torch.autograd.grad(out.sum(), f)
        errs = rel_l2(out, c["out"]), rel_l2(g, c["grad"])
        assert out.shape == c["out"].shape and max(errs) < 1e-6, (name, errs)
