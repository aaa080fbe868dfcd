"""GPU tests of RealVectorSHT / InverseRealVectorSHT (csrc/vlegendre.hip) and of the two losses built on them, against the
fp64 restatement of tests/_vsht_ref.py.  Gate of the transforms: the project's fp32 operator tolerance, rel-L2 <= 1e-5
 with three limbs; with two limbs (allow_tf32 = True) the scalar pair's gate, 2e-5."""
import os

import numpy as np
import pytest
import torch

import _vsht_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vsht_losses.npz")


def _pair(nlat, nlon, lmax, mmax, grid, matrices=ref.scipy_matrices):
    import makani_amd as ma
    kw = dict(lmax=lmax, mmax=mmax, grid=grid)
    return (ma.RealVectorSHT(nlat, nlon, **kw).to(DEV), ma.InverseRealVectorSHT(nlat, nlon, **kw).to(DEV),
            ref.RealVectorSHT(nlat, nlon, matrices=matrices, **kw), ref.InverseRealVectorSHT(nlat, nlon, matrices=matrices, **kw))


def _rand_coeffs(gen, lead, L, M):
    c = torch.complex(torch.randn(*lead, 2, L, M, generator=gen), torch.randn(*lead, 2, L, M, generator=gen))
    return ref.lower_triangle(c)


def _check_pair(fw, iv, rfw, riv, lead, gen, tol=TOL, tag=""):
    nlat, nlon, L, M = fw.nlat, fw.nlon, fw.lmax, fw.mmax
    # forward transform and its gradient under a random cotangent
    x = torch.randn(*lead, 2, nlat, nlon, generator=gen)
    ct = _rand_coeffs(gen, lead, L, M)
    xg = x.to(DEV).requires_grad_(True)
    y = fw(xg)
    assert y.shape == (*lead, 2, L, M) and y.dtype == torch.complex64
    (gx,) = torch.autograd.grad(y, xg, ct.to(DEV))
    xr = x.double().requires_grad_(True)
    yr = rfw(xr)
    (gxr,) = torch.autograd.grad(yr, xr, ct.to(torch.complex128))
    e = [ref.rel_l2(y, yr), ref.rel_l2(gx, gxr)]
    # inverse transform and its gradient
    c = _rand_coeffs(gen, lead, L, M)
    cx = torch.randn(*lead, 2, nlat, nlon, generator=gen)
    cg = c.to(DEV).requires_grad_(True)
    z = iv(cg)
    assert z.shape == (*lead, 2, nlat, nlon) and z.dtype == torch.float32
    (gc,) = torch.autograd.grad(z, cg, cx.to(DEV))
    cr = c.to(torch.complex128).requires_grad_(True)
    zr = riv(cr)
    (gcr,) = torch.autograd.grad(zr, cr, cx.double())
    e += [ref.rel_l2(z, zr), ref.rel_l2(ref.lower_triangle(gc.cpu()), ref.lower_triangle(gcr))]
    print(f"vsht {tag} {nlat}x{nlon} L={L} M={M} lead={tuple(lead)}: fwd {e[0]:.2e} fwd-grad {e[1]:.2e} inv {e[2]:.2e} inv-grad {e[3]:.2e}")
    assert max(e) <= tol, e
    return e


@pytest.mark.parametrize("nlat,nlon,lmax,mmax,grid,lead", [
    (33, 64, 33, 33, "equiangular", (3,)),              # poles on the grid, odd pair count
    (32, 64, 32, 33, "legendre-gauss", (2, 5)),         # lead shape that is not a multiple of the padding
    (31, 64, 30, 24, "lobatto", ()),                    # a single pair, truncated orders
    (64, 128, 40, 40, "equiangular", (35,)),            # more than one 32-row block of pairs
])
def test_vector_transforms_forward_and_backward_match_fp64(nlat, nlon, lmax, mmax, grid, lead):
    gen = torch.Generator().manual_seed(11)
    _check_pair(*_pair(nlat, nlon, lmax, mmax, grid), lead, gen)


def test_vector_transforms_under_both_settings_of_torchs_tf32_switch():
    from makani_amd import ops
    gen = torch.Generator().manual_seed(12)
    mods = _pair(120, 240, 120, 121, "legendre-gauss", matrices=ref.library_matrices)
    was = torch.backends.cuda.matmul.allow_tf32
    try:
        torch.backends.cuda.matmul.allow_tf32 = False
        assert ops.gemm_mode() == "x6"
        _check_pair(*mods, (4,), gen, tag="three limbs")
        torch.backends.cuda.matmul.allow_tf32 = True
        assert ops.gemm_mode() == "x3"
        _check_pair(*mods, (4,), gen, tol=2e-5, tag="two limbs")
    finally:
        torch.backends.cuda.matmul.allow_tf32 = was


def test_fullsize_vector_transforms_match_fp64():
    """721 x 1440, L = M = 721, three pairs; the fp64 side uses the library's own fp64 matrices (the scipy construction is
    quadratic in python calls; the two agree to 1e-12 at small sizes, tests/test_vsht_cpu.py)"""
    from makani_amd import legendre
    cache = {}

    def mats(mmax, lmax, theta):
        if "W" not in cache:
            cache["W"] = legendre.vector_legendre_matrices(mmax, lmax, theta)
        return cache["W"]

    gen = torch.Generator().manual_seed(13)
    _check_pair(*_pair(721, 1440, 721, 721, "equiangular", matrices=mats), (3,), gen, tag="full size")


def test_one_launch_equals_the_two_scalar_launch_composition():
    """s = W0^T U - i W1^T V, t = i W1^T U + W0^T V built from four scalar Legendre launches (ops.legendre_analysis with W0 and
    W1) and a combine pass — the thing the kernel replaces — agrees with the one-launch kernel to fp32 round-off"""
    import makani_amd as ma
    from makani_amd import ops
    fw = ma.RealVectorSHT(64, 128, lmax=64, mmax=65, grid="legendre-gauss").to(DEV)
    P = 7
    xc = torch.randn(2, P, 64, 128, device=DEV)
    Rp = ops.round32(P)
    F = ops.rfft_rows(xc, fw.mmax, Rp, fw._w)                       # (M, nlat, 2, 2 Rp)
    S = ops.vector_legendre(F, fw._mats(), 0)
    w0, w1 = fw.weights_t[0].contiguous(), fw.weights_t[1].contiguous()
    A0 = ops.legendre_analysis(F, w0, fw.lmax).view(fw.lmax, fw.mmax, 2, 2, Rp)
    A1 = ops.legendre_analysis(F, w1, fw.lmax).view(fw.lmax, fw.mmax, 2, 2, Rp)
    RE, IM, U, V = 0, 1, 0, 1
    want = torch.empty_like(A0)
    want[:, :, RE, 0] = A0[:, :, RE, U] + A1[:, :, IM, V]
    want[:, :, IM, 0] = A0[:, :, IM, U] - A1[:, :, RE, V]
    want[:, :, RE, 1] = -A1[:, :, IM, U] + A0[:, :, RE, V]
    want[:, :, IM, 1] = A1[:, :, RE, U] + A0[:, :, IM, V]
    got = S.view_as(want)
    tri = (torch.arange(fw.lmax, device=DEV)[:, None] >= torch.arange(fw.mmax, device=DEV)[None, :])[:, :, None, None, None]
    err = ref.rel_l2((got * tri)[..., :P], (want * tri)[..., :P])
    print(f"one launch vs composition: {err:.2e}")
    assert err <= 1e-6
    # ... and the s-only form equals the spheroidal half of the full one, bit for bit (same products in the same order)
    S2 = ops.vector_legendre(F, fw._mats(), 2).view(fw.lmax, fw.mmax, 2, Rp)
    assert torch.equal((S2 * tri[..., 0])[..., :P], (got[:, :, :, 0] * tri[..., 0])[..., :P])


def test_zero_toroidal_synthesis_equals_the_general_path_fed_zeros():
    import makani_amd as ma
    from makani_amd import ops
    iv = ma.InverseRealVectorSHT(33, 64, lmax=33, mmax=33, grid="equiangular").to(DEV)
    P = 5
    Rp = ops.round32(P)
    s = torch.randn(33, 33, 2, Rp, device=DEV)
    full = torch.zeros(33, 33, 2, 2, Rp, device=DEV)
    full[:, :, :, 0] = s
    a = iv.synthesis(s, P, t_zero=True)
    b = iv.synthesis(full.view(33, 33, 2, 2 * Rp), P)
    assert a.shape == (2, P, 33, 64)
    err = float((a - b).abs().max() / b.abs().max())
    print(f"t = 0 synthesis vs explicit zeros: {err:.2e}")
    assert err <= 1e-7


def test_kernels_replay_from_a_captured_graph():
    import makani_amd as ma
    fw = ma.RealVectorSHT(33, 64, grid="equiangular").to(DEV)
    iv = ma.InverseRealVectorSHT(33, 64, grid="equiangular").to(DEV)
    x = torch.randn(3, 2, 33, 64, device=DEV)
    eager = iv(fw(x))                                   # also warms up plans, limb planes and bands outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            out = iv(fw(x))
    torch.cuda.current_stream().wait_stream(stream)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ----------------------------------------------------------------------------------------------------------------------
# losses against the fixtures recorded from the reference's own classes (tools/make_vsht_golden.py)
# ----------------------------------------------------------------------------------------------------------------------
def _cases():
    if not os.path.exists(GOLDEN):
        return []
    with np.load(GOLDEN) as z:
        return sorted({k.split("/")[0] for k in z.files})


@pytest.mark.parametrize("case", _cases() or ["missing"])
def test_losses_match_the_reference_fixtures(case):
    """value and forecast gradient of both losses, rel-L2 <= 1e-5 as tests/test_crps.py gates CRPSLoss.  The absolute-gradient
    cases differentiate sqrt(g_theta^2 + g_phi^2): the recorded inputs are smooth fields plus an O(1) offset gradient, so the
    magnitude stays away from zero except at isolated points (the fixture generator prints the smallest magnitude)."""
    import json
    import makani_amd as ma
    assert case != "missing", "tests/golden/vsht_losses.npz is not there"
    z = np.load(GOLDEN)
    meta = json.loads(str(z[f"{case}/meta"]))
    cls = getattr(ma, meta["cls"])
    loss = cls(**meta["kwargs"]).to(DEV)
    f = torch.from_numpy(z[f"{case}/forecasts"]).to(DEV).requires_grad_(True)
    o = torch.from_numpy(z[f"{case}/observations"]).to(DEV)
    w = torch.from_numpy(z[f"{case}/weights"]).to(DEV) if f"{case}/weights" in z.files else None
    out = loss(f, o, w)
    want = torch.from_numpy(z[f"{case}/out"])
    assert out.shape == want.shape
    (gf,) = torch.autograd.grad(out.sum(), f)
    ev, eg = ref.rel_l2(out, want), ref.rel_l2(gf, torch.from_numpy(z[f"{case}/grad"]))
    print(f"{case}: value {ev:.2e} gradient {eg:.2e}")
    assert ev <= 1e-5 and eg <= 1e-5


NAMES = ["u500", "v500", "u850", "v850", "t500"]
KW = dict(img_shape=(33, 64), crop_shape=(33, 64), crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")


@pytest.mark.parametrize("cls,nout", [("GradientCRPSLoss", 5), ("VortDivCRPSLoss", 5)])
def test_losses_take_bf16_and_keep_the_transforms_in_fp32(cls, nout):
    import makani_amd as ma
    loss = getattr(ma, cls)(**KW).to(DEV)
    gen = torch.Generator().manual_seed(5)
    f = torch.randn(2, 3, 5, 33, 64, generator=gen).to(DEV)
    o = torch.randn(2, 5, 33, 64, generator=gen).to(DEV)
    full = loss(f, o)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        half = loss(f.bfloat16(), o.bfloat16())
    assert half.shape == (2, nout) and half.dtype == torch.float32 and torch.isfinite(half).all()
    # bf16 rounding of the inputs (and, for the gradient loss, of the transformed fields: 2^-9 per value), not of the transforms
    assert ref.rel_l2(half, full) < 2e-2


def test_gradient_loss_has_finite_gradients_at_a_perfect_forecast():
    import makani_amd as ma
    loss = ma.GradientCRPSLoss(**KW).to(DEV)
    o = torch.randn(1, 5, 33, 64, generator=torch.Generator().manual_seed(6)).to(DEV)
    f = o.unsqueeze(1).repeat(1, 2, 1, 1, 1).requires_grad_(True)
    out = loss(f, o)
    (g,) = torch.autograd.grad(out.sum(), f)
    assert torch.isfinite(out).all() and torch.isfinite(g).all()
