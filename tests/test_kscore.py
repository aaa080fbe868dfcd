"""KernelScoreLoss on the host: constructor attributes and buffers, the reference's error messages, the stated refusals."""
import math

import pytest
import torch

import makani_amd as ma
from makani_amd import losses

SHAPE = (13, 24)


def _loss(**kw):
    kw = {"kernel_basis_type": "morlet", "kernel_basis_norm_mode": "mean", **kw}
    return ma.KernelScoreLoss(SHAPE, SHAPE, (0, 0), ["u", "v", "t"], "equiangular", **kw)


def test_attributes_and_buffers():
    w = torch.tensor([1.0, 2.0, 3.0])
    loss = _loss(crps_type="cdf", ensemble_weights=w, kernel_shape=(3, 3), unknown_keyword=1)
    assert loss.type == "probabilistic" and loss.n_channels == 3 and loss.kernel_basis_size == 9
    assert loss.theta_cutoff == 2 * 3 * math.pi / 12
    assert loss.quad_weight_split.shape == (1, 1, 13 * 24) and torch.equal(loss.ensemble_weights, w)
    assert not loss.state_dict()                                   # both buffers are non-persistent
    assert _loss().ensemble_weights is None
    assert _loss(kernel_basis_type="zernike", kernel_shape=(3,)).kernel_basis_size == 6
    assert _loss(kernel_basis_type="piecewise linear", kernel_shape=(3, 2)).kernel_basis_size == 3


def test_exported_but_not_registered():
    assert "KernelScoreLoss" in ma.__all__
    assert all(v is not ma.KernelScoreLoss for v in losses._LOSS_REGISTRY.values()) and "KernelScoreLoss" not in str(losses._LOSS_REGISTRY)


def test_error_messages():
    loss = _loss()
    f, o = torch.zeros(2, 4, 3, 13, 24), torch.zeros(2, 3, 13, 24)
    with pytest.raises(ValueError, match="forecasts tensor expected to have 5 dimensions but found 4"):
        loss(f[0], o)
    with pytest.raises(ValueError, match=r"same number of dimensions \(found 3\) as observations \(found 4\)"):
        loss(f, o, torch.ones(3, 13, 24))
    with pytest.raises(NotImplementedError, match="alpha parameter .* only supported for the skillspread kernels"):
        _loss(crps_type="cdf", alpha=0.9)
    with pytest.raises(ValueError, match="batch extent 1 or 2, channel extent 1 or 27"):
        loss(f, o, torch.ones(2, 3, 13, 24))
    with pytest.raises(ValueError, match="ensemble_weights must be finite"):
        _loss(crps_type="cdf", ensemble_weights=torch.tensor([1.0, float("nan")]))


def test_refusals():
    with pytest.raises(NotImplementedError, match="filter basis 'harmonic'"):
        ma.KernelScoreLoss(SHAPE, SHAPE, (0, 0), ["u"], "equiangular")              # the reference's defaults
    with pytest.raises(ValueError, match="Unknown basis normalization mode nodal"):
        _loss(kernel_basis_norm_mode="nodal")
    loss = _loss()
    with pytest.raises(NotImplementedError, match="ensemble size 33"):
        loss(torch.zeros(1, 33, 3, 13, 24), torch.zeros(1, 3, 13, 24))
    with pytest.raises(RuntimeError, match="GPU"):
        loss(torch.zeros(1, 2, 3, 13, 24), torch.zeros(1, 3, 13, 24))
