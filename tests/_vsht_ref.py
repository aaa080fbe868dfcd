"""Test-side fp64 restatement of the vector spherical harmonic transform pair (dense torch: ``fft.rfft`` + ``einsum``), the
reference every vector-SHT test compares against.  The latitude functions are built from ``scipy.special.sph_harm_y``
INDEPENDENTLY of ``makani_amd/legendre.py``: d P/d theta is scipy's own analytic theta-derivative, m P/sin(theta) comes
from the degree-(l + 1) identity (legendre.py uses the degree-(l - 1) one), so neither divides by sin(theta) at the poles.

Convention (the one ``legendre.vector_legendre_matrices`` documents): Psi_lm = grad Y_lm / sqrt(l (l + 1)),
Phi_lm = r x Psi_lm, field = sum s_lm Psi_lm + t_lm Phi_lm, component 0 = theta-hat, component 1 = phi-hat.
"""
import math

import numpy as np
import torch


def scipy_matrices(mmax, lmax, theta):
    """(2, mmax, lmax, nlat) fp64, orthonormal, Condon-Shortley phase: [dP/dtheta, m P/sin(theta)] / sqrt(l (l + 1))"""
    from scipy.special import sph_harm_y
    th = np.asarray(theta, dtype=np.float64)
    W = np.zeros((2, mmax, lmax, len(th)))

    def P(l, m):                                    # orthonormal P_l^m(theta) = Y_l^m(theta, 0); zero for m > l
        if m > l or m < 0:
            return np.zeros_like(th)
        return sph_harm_y(l, m, th, 0.0).real

    for l in range(1, lmax):
        for m in range(min(mmax, l + 1)):
            _, g = sph_harm_y(l, m, th, 0.0, diff_n=1)
            W[0, m, l] = g[..., 0].real
            if m > 0:
                W[1, m, l] = -0.5 * math.sqrt((2 * l + 1) / (2 * l + 3)) * (
                    math.sqrt((l - m + 1) * (l - m + 2)) * P(l + 1, m - 1) + math.sqrt((l + m + 1) * (l + m + 2)) * P(l + 1, m + 1))
        W[:, :, l] /= math.sqrt(l * (l + 1))
    return W


def library_matrices(mmax, lmax, theta):
    """the library's own fp64 matrices — for sizes where the scipy construction takes too long (its agreement with
    ``scipy_matrices`` to 1e-12 is what tests/test_vsht_cpu.py checks at small sizes)"""
    from makani_amd import legendre
    return legendre.vector_legendre_matrices(mmax, lmax, theta)


def grid(nlat, kind):
    from makani_amd import legendre
    return legendre.colatitudes(nlat, kind)


class RealVectorSHT(torch.nn.Module):
    """(..., 2, nlat, nlon) -> (..., 2, lmax, mmax) complex128; any real input dtype (computed in fp64)"""

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True, matrices=scipy_matrices):
        super().__init__()
        assert norm == "ortho" and csphase
        self.nlat, self.nlon, self.grid = nlat, nlon, grid
        self.lmax = lmax or (nlat - 1 if grid == "lobatto" else nlat)
        self.mmax = mmax or nlon // 2 + 1
        theta, wq = globals()["grid"](nlat, grid)
        W = matrices(self.mmax, self.lmax, theta)
        self.register_buffer("weights", torch.from_numpy(W * wq[None, None, None, :]), persistent=False)

    def forward(self, x):
        X = 2.0 * math.pi * torch.fft.rfft(x.to(torch.float64), dim=-1, norm="forward")[..., : self.mmax]
        U, V = X[..., 0, :, :], X[..., 1, :, :]
        W0, W1 = self.weights[0].to(X.dtype), self.weights[1].to(X.dtype)
        s = torch.einsum("mlk,...km->...lm", W0, U) - 1j * torch.einsum("mlk,...km->...lm", W1, V)
        t = 1j * torch.einsum("mlk,...km->...lm", W1, U) + torch.einsum("mlk,...km->...lm", W0, V)
        return torch.stack([s, t], dim=-3)


class InverseRealVectorSHT(torch.nn.Module):
    """(..., 2, lmax, mmax) complex -> (..., 2, nlat, nlon) fp64"""

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True, matrices=scipy_matrices):
        super().__init__()
        assert norm == "ortho" and csphase
        self.nlat, self.nlon, self.grid = nlat, nlon, grid
        self.lmax = lmax or (nlat - 1 if grid == "lobatto" else nlat)
        self.mmax = mmax or nlon // 2 + 1
        theta, _ = globals()["grid"](nlat, grid)
        self.register_buffer("pct", torch.from_numpy(matrices(self.mmax, self.lmax, theta)), persistent=False)

    def forward(self, c):
        c = c.to(torch.complex128)
        s, t = c[..., 0, :, :], c[..., 1, :, :]
        W0, W1 = self.pct[0].to(c.dtype), self.pct[1].to(c.dtype)
        U = torch.einsum("mlk,...lm->...km", W0, s) - 1j * torch.einsum("mlk,...lm->...km", W1, t)
        V = 1j * torch.einsum("mlk,...lm->...km", W1, s) + torch.einsum("mlk,...lm->...km", W0, t)
        X = torch.stack([U, V], dim=-3)
        return torch.fft.irfft(X, n=self.nlon, dim=-1, norm="forward")


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach(), torch.as_tensor(b).detach()
    a = a.to(torch.complex128 if a.is_complex() else torch.float64).cpu()
    b = b.to(a.dtype).cpu()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-300))


def lower_triangle(c):
    """zero the l < m entries (the transforms never produce them)"""
    L, M = c.shape[-2:]
    keep = (torch.arange(L)[:, None] >= torch.arange(M)[None, :]).to(c.device)
    return c * keep
