"""Host-side (numpy, fp64) precompute for the spherical harmonic transforms:
quadrature nodes / weights and the normalised associated Legendre functions.

Same mathematical objects as torch-harmonics' ``quadrature`` /
``legendre._precompute_legpoly`` [un-vendored; used by the reference at
``makani/models/networks/sfnonet.py:802-805``], computed here with a recurrence
vectorised over (m, latitude) per degree.  Runs once per transform object.
"""
import math

import numpy as np


def gauss_legendre(n):
    """nodes cos(theta) ascending in [-1, 1] and weights (sum = 2)."""
    x, w = np.polynomial.legendre.leggauss(n)
    return x, w


def clenshaw_curtis(n):
    """Clenshaw-Curtis rule on the equiangular grid cos(j*pi/(n-1)) incl. both poles.

    Weights from the closed form  w_j = c_j/(n-1) * (1 - sum_k b_k/(4k^2-1) cos(2 k j pi/(n-1)))
    evaluated through one FFT (Waldvogel's construction)."""
    if n < 2:
        raise ValueError("equiangular grid needs nlat >= 2")
    x = np.cos(np.linspace(np.pi, 0.0, n))
    if n == 2:
        return x, np.array([1.0, 1.0])
    n1 = n - 1
    odd = np.arange(1, n1, 2)
    nodd = len(odd)
    rest = n1 - nodd
    v = np.concatenate([2.0 / odd / (odd - 2), 1.0 / odd[-1:], np.zeros(rest)])
    v = -v[:-1] - v[-1:0:-1]
    g = -np.ones(n1)
    g[nodd] += n1
    g[rest] += n1
    g /= n1 * n1 - 1 + (n1 % 2)
    w = np.fft.ifft(v + g).real
    return x, np.concatenate([w, w[:1]])


def gauss_lobatto(n, tol=1e-16, maxiter=100):
    x = -np.cos(np.pi * np.arange(n) / (n - 1))
    P = np.zeros((n, n))
    for _ in range(maxiter):
        xo = x
        P[:, 0] = 1.0
        P[:, 1] = x
        for k in range(2, n):
            P[:, k] = ((2 * k - 1) * x * P[:, k - 1] - (k - 1) * P[:, k - 2]) / k
        x = xo - (x * P[:, n - 1] - P[:, n - 2]) / (n * P[:, n - 1])
        if np.max(np.abs(x - xo)) < tol:
            break
    w = 2.0 / (n * (n - 1) * P[:, n - 1] ** 2)
    return x, w


def grid_nodes(nlat, grid):
    if grid == "legendre-gauss":
        return gauss_legendre(nlat)
    if grid == "equiangular":
        return clenshaw_curtis(nlat)
    if grid == "lobatto":
        return gauss_lobatto(nlat)
    raise ValueError(f"Unknown quadrature mode {grid}")


def colatitudes(nlat, grid):
    """(theta ascending from the north pole, quadrature weights in the same order)."""
    x, w = grid_nodes(nlat, grid)
    return np.flip(np.arccos(x)).copy(), np.flip(w).copy()


def legendre_matrix(mmax, lmax, theta, norm="ortho", inverse=False, csphase=True):
    """P[m, l, k] (fp64): orthonormal associated Legendre functions at colatitudes theta[k]."""
    n = max(mmax, lmax)
    x = np.cos(theta)
    nk = len(theta)
    P = np.zeros((n, n, nk))
    nf = 1.0 if norm == "ortho" else math.sqrt(4 * math.pi)
    if inverse:
        nf = 1.0 / nf
    P[0, 0] = nf / math.sqrt(4 * math.pi)
    s2 = (1.0 + x) * (1.0 - x)
    for l in range(1, n):
        P[l, l] = np.sqrt((2 * l + 1) * s2 / (2 * l)) * P[l - 1, l - 1]
        P[l - 1, l] = math.sqrt(2 * l + 1) * x * P[l - 1, l - 1]
    for l in range(2, n):
        m = np.arange(0, l - 1, dtype=np.float64)[:, None]
        a = np.sqrt((2 * l - 1) / (l - m) * (2 * l + 1) / (l + m))
        b = np.sqrt((l + m - 1) / (l - m) * (2 * l + 1) / (2 * l - 3) * (l - m - 1) / (l + m))
        P[: l - 1, l] = a * x[None, :] * P[: l - 1, l - 1] - b * P[: l - 1, l - 2]
    if norm == "schmidt":
        f = np.sqrt(2.0 * np.arange(n) + 1.0)[None, :, None]
        P = P * f if inverse else P / f
    P = P[:mmax, :lmax]
    if csphase:
        P[1::2] *= -1.0
    return P


def vector_legendre_matrices(mmax, lmax, theta, norm="ortho", inverse=False, csphase=True):
    """W[c, m, l, k] (fp64, (2, mmax, lmax, nlat)): the two latitude functions of the vector spherical harmonic transforms,

        W[0] = d P_l^m / d theta / sqrt(l (l + 1))          W[1] = m P_l^m / sin(theta) / sqrt(l (l + 1))

    with P_l^m of ``legendre_matrix`` (same ``norm`` / ``inverse`` / ``csphase``); row l = 0 is zero (a constant has no
    gradient).  Convention (the orthonormal vector harmonics; the published torch-harmonics ``RealVectorSHT`` pair is
    not available to compare against, so the convention is pinned by mathematics in tests/test_vsht_cpu.py):
    with Y_lm = P_l^m(theta) e^{i m phi},

        Psi_lm = grad Y_lm / sqrt(l (l + 1))   (spheroidal),      Phi_lm = r x Psi_lm   (toroidal),

    a tangent field with components (component 0 = colatitudinal theta-hat, pointing SOUTH; component 1 = azimuthal
    phi-hat, pointing EAST) is  sum_lm  s_lm Psi_lm + t_lm Phi_lm, i.e. per order m and with U, V the longitude spectra
    of the two components (Psi = (W0, i W1), Phi = (-i W1, W0))

        U = W0 s - i W1 t             s = W0^T U - i W1^T V
        V = i W1 s + W0 t             t = i W1^T U + W0^T V          (^T: quadrature over latitude)

    so that ``ivsht([f_lm sqrt(l (l + 1)), 0])`` is the surface gradient (d/dtheta, 1/sin(theta) d/dphi) of the scalar
    field with coefficients f_lm, a field with s = 0 is divergence free and one with t = 0 curl free.  The sign of the
    toroidal part: t_lm multiplies +Phi_lm = +r x Psi_lm (r x theta-hat = phi-hat), so the stream function psi with
    coefficients t_lm / sqrt(l (l + 1)) gives the field r x grad psi and the vorticity  -sum sqrt(l (l + 1)) t_lm Y_lm.

    Both functions are evaluated WITHOUT a division by sin(theta) (the equiangular grids have nodes at both poles), from
    the orthonormal functions of the neighbouring orders (ladder operators; Condon-Shortley phase included):

        d P_l^m / d theta  = ( sqrt((l - m)(l + m + 1)) P_l^{m+1} - sqrt((l + m)(l - m + 1)) P_l^{m-1} ) / 2
        m P_l^m / sin      = - sqrt((2l + 1) / (2l - 1)) ( sqrt((l - m)(l - m - 1)) P_{l-1}^{m+1}
                                                           + sqrt((l + m)(l + m - 1)) P_{l-1}^{m-1} ) / 2
    with P_l^{-1} = -P_l^1."""
    n = max(mmax + 1, lmax)
    P = legendre_matrix(n, n, theta, norm="ortho", inverse=False, csphase=True)       # (order, degree, latitude)
    nk = len(theta)
    W = np.zeros((2, mmax, lmax, nk))
    l = np.arange(lmax, dtype=np.float64)[:, None]
    Pl = P[:, :lmax]                                                                   # degree l

    def below(m):                                                                      # P_{l-1}^m as a function of l
        out = np.zeros((lmax, nk))
        out[1:] = P[m, : lmax - 1]
        return out

    for m in range(mmax):
        up = Pl[m + 1]
        dn = Pl[m - 1] if m > 0 else -Pl[1]
        cp = np.sqrt(np.maximum((l - m) * (l + m + 1), 0.0))
        cm = np.sqrt(np.maximum((l + m) * (l - m + 1), 0.0))
        W[0, m] = 0.5 * (cp * up - cm * dn)
        if m > 0:
            ap = np.sqrt(np.maximum((l - m) * (l - m - 1), 0.0))
            am = np.sqrt(np.maximum((l + m) * (l + m - 1), 0.0))
            f = np.sqrt((2 * l + 1) / np.maximum(2 * l - 1, 1.0))
            W[1, m] = -0.5 * f * (ap * below(m + 1) + am * below(m - 1))
        W[:, m, : min(m, lmax)] = 0.0                                                  # l < m
    ll = np.arange(lmax, dtype=np.float64)
    scale = np.zeros(lmax)
    scale[1:] = 1.0 / np.sqrt(ll[1:] * (ll[1:] + 1.0))
    nf = 1.0 if norm == "ortho" else math.sqrt(4 * math.pi)                            # as legendre_matrix
    if inverse:
        nf = 1.0 / nf
    scale *= nf
    if norm == "schmidt":
        f = np.sqrt(2.0 * ll + 1.0)
        scale = scale * f if inverse else scale / f
    W *= scale[None, None, :, None]
    if not csphase:
        W[:, 1::2] *= -1.0
    return W


def factorize_half(nlon):
    """Radix list (4s first, then 2, 3, 5, small primes) whose product is nlon // 2."""
    if nlon % 2:
        raise NotImplementedError(f"nlon={nlon}: odd longitude counts are not supported by the HIP FFT")
    n = nlon // 2
    out = []
    while n % 4 == 0:
        out.append(4)
        n //= 4
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
        while n % p == 0:
            out.append(p)
            n //= p
    if n != 1:
        raise NotImplementedError(f"nlon={nlon}: prime factor > 31 is not supported by the HIP FFT")
    return out or [1]


def twiddle_table(nlon):
    """exp(-2 pi i q / nlon), q < nlon, as (nlon, 2) float32 (rounded from fp64)."""
    q = np.arange(nlon, dtype=np.float64)
    a = -2.0 * np.pi * q / nlon
    return np.stack([np.cos(a), np.sin(a)], axis=-1).astype(np.float32)
