"""CPU tests of the vector spherical harmonic transform pair: the host precompute against scipy, the fp64 restatement
(tests/_vsht_ref.py) pinned by mathematics, and the constructor contracts of the modules and the two losses."""
import math

import numpy as np
import pytest
import torch

import _vsht_ref as ref


@pytest.mark.parametrize("grid,nlat", [("equiangular", 17), ("legendre-gauss", 16), ("lobatto", 15)])
def test_vector_legendre_matrices_match_scipy_including_the_poles(grid, nlat):
    from makani_amd import legendre
    theta, _ = legendre.colatitudes(nlat, grid)
    lmax = nlat - 1 if grid == "lobatto" else nlat
    mmax = lmax
    W = legendre.vector_legendre_matrices(mmax, lmax, theta)
    R = ref.scipy_matrices(mmax, lmax, theta)
    assert W.shape == (2, mmax, lmax, nlat) and W.dtype == np.float64
    assert np.isfinite(W).all()
    if grid != "legendre-gauss":
        assert theta[0] < 1e-7 and abs(theta[-1] - math.pi) < 1e-7          # the poles are nodes
    err = np.abs(W - R).max()
    print(f"{grid}: max |W - scipy| = {err:.3e}")
    assert err <= 1e-12
    assert (W[:, :, 0] == 0.0).all()
    # the other normalisations and the phase follow legendre_matrix
    P = legendre.legendre_matrix(mmax, lmax, theta, norm="schmidt", inverse=True, csphase=False)
    Po = legendre.legendre_matrix(mmax, lmax, theta)
    Ws = legendre.vector_legendre_matrices(mmax, lmax, theta, norm="schmidt", inverse=True, csphase=False)
    l, m = 5, 3
    k = nlat // 3
    assert np.allclose(Ws[:, m, l, k] * Po[m, l, k], W[:, m, l, k] * P[m, l, k], rtol=1e-12, atol=0)


def _pair(nlat, nlon, grid, lmax):
    return (ref.RealVectorSHT(nlat, nlon, lmax=lmax, mmax=lmax, grid=grid), ref.InverseRealVectorSHT(nlat, nlon, lmax=lmax, mmax=lmax, grid=grid))


def _coeffs(gen, shape, L):
    c = torch.complex(torch.randn(*shape, L, L, generator=gen, dtype=torch.float64), torch.randn(*shape, L, L, generator=gen, dtype=torch.float64))
    c = ref.lower_triangle(c)
    c[..., :, 0] = c[..., :, 0].real.to(c.dtype)              # a real field has real m = 0 coefficients
    return c


def test_restatement_gradient_of_a_bandlimited_scalar_is_the_analytic_surface_gradient():
    from scipy.special import sph_harm_y
    nlat, nlon, L = 16, 32, 12
    _, iv = _pair(nlat, nlon, "legendre-gauss", L)
    theta, _ = ref.grid(nlat, "legendre-gauss")
    phi = 2 * math.pi * np.arange(nlon) / nlon
    f = _coeffs(torch.Generator().manual_seed(1), (), L)
    ll = torch.arange(L, dtype=torch.float64)[:, None]
    c = torch.stack([f * torch.sqrt(ll * (ll + 1)), torch.zeros_like(f)])
    got = iv(c).numpy()
    T, Ph = np.meshgrid(theta, phi, indexing="ij")
    want = np.zeros((2, nlat, nlon))
    for l in range(L):
        for m in range(l + 1):
            y, g = sph_harm_y(l, m, T, Ph, diff_n=1)
            w = 1.0 if m == 0 else 2.0
            flm = complex(f[l, m])
            want[0] += w * (flm * g[..., 0]).real
            want[1] += w * (flm * g[..., 1]).real / np.sin(T)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"gradient: {err:.3e}")
    assert err <= 1e-10


def test_restatement_round_trip_purity_and_parseval_on_the_gauss_grid():
    nlat, nlon, L = 16, 32, 12
    fw, iv = _pair(nlat, nlon, "legendre-gauss", L)
    gen = torch.Generator().manual_seed(2)
    c = _coeffs(gen, (3, 2), L)
    c[..., 0, :] = 0                                            # degree 0 carries no vector field
    x = iv(c)
    back = fw(x)
    err = ref.rel_l2(back, c)
    print(f"round trip: {err:.3e}")
    assert err <= 1e-10
    # a pure-toroidal field has no spheroidal (divergence) coefficients and vice versa
    tor = c.clone()
    tor[:, 0] = 0
    sph = c.clone()
    sph[:, 1] = 0
    assert float(fw(iv(tor))[:, 0].abs().max()) <= 1e-10
    assert float(fw(iv(sph))[:, 1].abs().max()) <= 1e-10
    # Parseval with the quadrature weights: int |F|^2 = sum_m w(m) (|s|^2 + |t|^2)
    _, wq = ref.grid(nlat, "legendre-gauss")
    lhs = (x.pow(2).sum(dim=1) * torch.from_numpy(wq)[:, None]).sum(dim=(-2, -1)) * (2 * math.pi / nlon)
    wm = torch.full((L,), 2.0, dtype=torch.float64)
    wm[0] = 1.0
    rhs = (c.abs().pow(2).sum(dim=1) * wm).sum(dim=(-2, -1))
    assert torch.allclose(lhs, rhs, rtol=1e-10, atol=0)


def test_module_contracts():
    import makani_amd as ma
    fw = ma.RealVectorSHT(17, 32, lmax=12, mmax=10)
    iv = ma.InverseRealVectorSHT(17, 32, lmax=12, mmax=10)
    for mod, names in ((fw, ("weights", "weights_t")), (iv, ("pct", "pct_t"))):
        assert (mod.nlat, mod.nlon, mod.lmax, mod.mmax, mod.grid, mod.norm, mod.csphase) == (17, 32, 12, 10, "equiangular", "ortho", True)
        assert len(mod.state_dict()) == 0                         # non-persistent buffers only
        assert getattr(mod, names[0]).shape == (2, 10, 12, 20) and getattr(mod, names[1]).shape == (2, 10, 17, 12)
        assert getattr(mod, names[0]).dtype == torch.float32
    assert ma.RealVectorSHT(15, 32, grid="lobatto").lmax == 14
    with pytest.raises(ValueError):
        ma.RealVectorSHT(17, 32, mmax=18)
    with pytest.raises(ValueError):
        ma.RealVectorSHT(17, 32, grid="healpix")
    with pytest.raises(NotImplementedError):
        ma.InverseRealVectorSHT(17, 31)
    with pytest.raises(TypeError):
        fw(torch.zeros(2, 17, 32, dtype=torch.float64))
    with pytest.raises(ValueError):
        fw(torch.zeros(3, 17, 32))
    with pytest.raises(ValueError):
        fw(torch.zeros(2, 16, 32))
    with pytest.raises(TypeError):
        iv(torch.zeros(2, 12, 10))
    with pytest.raises(ValueError):
        iv(torch.zeros(2, 12, 9, dtype=torch.complex64))
    with pytest.raises(RuntimeError):                             # no CPU implementation behind the modules
        fw(torch.zeros(2, 17, 32))


NAMES = ["u500", "v500", "u850", "v850", "t500"]


def test_loss_contracts(monkeypatch):
    import makani_amd as ma
    from makani_amd import comm
    kw = dict(img_shape=(17, 32), crop_shape=(17, 32), crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")
    g = ma.GradientCRPSLoss(**kw)
    assert g.absolute and g.n_channels == 5 and g.type == "probabilistic" and g.crps_type == "skillspread"
    g2 = ma.GradientCRPSLoss(absolute=False, **kw)
    assert g2.n_channels == 10
    v = ma.VortDivCRPSLoss(**kw)
    assert v.n_channels == 5 and v.wind_chans.tolist() == [0, 1, 2, 3] and v.type == "probabilistic"
    assert ma.VortDivCRPSLoss(**{**kw, "channel_names": ["v10m", "t2m", "u10m", "u100m"]}).wind_chans.tolist() == [2, 0]
    assert len(g.state_dict()) == 0 and len(v.state_dict()) == 0
    for cls in (ma.GradientCRPSLoss, ma.VortDivCRPSLoss):
        with pytest.raises(NotImplementedError):
            cls(crps_type="cdf", alpha=0.5, **kw)
        serial = cls(spatial_distributed=True, ensemble_distributed=True, **kw)     # no group larger than one: the flags are moot
        assert not serial.spatial_distributed and not serial.ensemble_distributed
        with monkeypatch.context() as mp:                                            # a process-group tree with split groups
            mp.setattr(comm, "autodetect", lambda: None)
            mp.setattr(comm, "is_distributed", lambda name: True)
            mp.setattr(comm, "get_size", lambda name: 2)
            with pytest.raises(NotImplementedError, match="distributed"):
                cls(spatial_distributed=True, **kw)
            with pytest.raises(NotImplementedError, match="distributed"):
                cls(ensemble_distributed=True, **kw)
            cls(**kw)                                                                # flags off: fine on any tree
        with pytest.raises(NotImplementedError):
            cls(crps_type="skillspread", ensemble_weights=torch.ones(4), **kw)
        loss = cls(**kw)
        with pytest.raises(ValueError, match="5 dimensions"):
            loss(torch.zeros(1, 5, 17, 32), torch.zeros(1, 5, 17, 32))
        with pytest.raises(ValueError, match="same number of dimensions"):
            loss(torch.zeros(1, 2, 5, 17, 32), torch.zeros(1, 5, 17, 32), torch.zeros(17, 32))
        bad = cls(**kw)
        bad.crps_type = "nonsense"
        with pytest.raises((ValueError, RuntimeError)):
            bad(torch.zeros(1, 2, 5, 17, 32), torch.zeros(1, 5, 17, 32))


def test_channel_weighting_averages_the_wind_pairs():
    import makani_amd as ma
    kw = dict(img_shape=(17, 32), crop_shape=(17, 32), crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")
    v = ma.VortDivCRPSLoss(**kw)
    base = torch.tensor([1.0, 3.0, 2.0, 6.0, 5.0])
    out = v.average_wind_weights(base.clone())
    assert out.tolist() == [2.0, 2.0, 4.0, 4.0, 5.0]
    g = ma.GradientCRPSLoss(absolute=False, **kw)
    assert [float(w) for w in g.expand_channel_weights(base)] == [1.0, 1.0, 3.0, 3.0, 2.0, 2.0, 6.0, 6.0, 5.0, 5.0]
