"""Multi-process CPU tests (gloo, 127.0.0.1) of the h x w schedule of the distributed vector transform pair
(makani_amd/distributed.py: DistributedRealVectorSHT / DistributedInverseRealVectorSHT) in the pattern of
tests/test_distributed_cpu.py: the local compute is injected as torch fp64 stand-ins for the backend hooks (FFT, the vector
Legendre launch of modes 0-3, the column-block repack), the exchanges are the product code, and every rank compares its shard
with the serial fp64 pair of tests/_vsht_ref.py, forward and backward, at the gate of the scalar schedule test (1e-5 absolute,
relative to the largest reference entry where that exceeds one).  Also the constructor contracts of the two losses on a real
process-group tree."""
import torch

from _ranks import launch, ranks

GATE = 1e-5


def _round32(n):
    return (n + 31) // 32 * 32


class VectorOracleBackend:
    """torch stand-ins on the internal layouts: F (M, nlat, 2, B * Cp), S (L, M, 2, blocks / 2 * Rp)"""

    @staticmethod
    def _wv(M, nlon, w, dtype):
        wv = torch.full((M,), w[1], dtype=dtype)
        wv[0] = w[0]
        if M - 1 == nlon // 2:
            wv[-1] = w[2]
        return wv

    @staticmethod
    def rfft(x4, mmax, w, Cp=None):
        B, P, nlat, nlon = x4.shape
        Cp = P + (-P) % 4 if Cp is None else Cp
        X = torch.fft.rfft(x4, dim=-1, norm="backward")[..., :mmax] * VectorOracleBackend._wv(mmax, nlon, w, x4.dtype)
        F = torch.stack([X.real, X.imag], dim=0).permute(4, 3, 0, 1, 2)                  # (M, nlat, 2, B, P)
        return torch.nn.functional.pad(F, (0, Cp - P)).reshape(mmax, nlat, 2, B * Cp)

    @staticmethod
    def irfft(F, planes, nlon, dtype, w, B=1):
        M, nlat = F.shape[:2]
        Fv = F.reshape(M, nlat, 2, B, -1)[..., :planes]
        X = torch.complex(Fv[:, :, 0], Fv[:, :, 1]).permute(2, 3, 1, 0)                  # (B, P, nlat, M)
        s = torch.full((M,), 2.0, dtype=F.dtype)
        s[0] = 1.0
        mask = torch.ones(M, dtype=F.dtype)
        mask[0] = 0.0
        if M - 1 == nlon // 2:
            s[-1], mask[-1] = 1.0, 0.0
        X = torch.complex(X.real, X.imag * mask) * (VectorOracleBackend._wv(M, nlon, w, F.dtype) / s)
        return torch.fft.irfft(X, n=nlon, dim=-1, norm="forward").to(dtype)

    @staticmethod
    def vlegendre(X, vm, mode, m_off):
        """csrc/vlegendre.hip in complex fp64: modes 0 / 2 read vm.tr (M_loc, nlat, lp), modes 1 / 3 vm.nat (M_loc, L, kp)"""
        ana = mode in (0, 2)
        nin = 1 if mode == 3 else 2
        a, b = X.shape[:2]
        Xv = X.reshape(a, b, 2, nin, -1)
        Z = torch.complex(Xv[:, :, 0], Xv[:, :, 1])                                        # (a, b, nin, Rp)
        assert (vm.tr if ana else vm.nat)[0].shape[0] == (a if ana else b), "the matrices must hold this rank's orders"
        if ana:                                                                            # X = F (M, nlat, ..)
            A0, A1 = (t[:, :, :vm.L].to(Z.dtype) for t in vm.tr)
            mul = lambda A, z: torch.einsum("mkl,mkr->lmr", A, z)
        else:                                                                              # X = S (L, M, ..)
            A0, A1 = (t[:, :, :vm.nlat].to(Z.dtype) for t in vm.nat)
            mul = lambda A, z: torch.einsum("mlk,lmr->mkr", A, z)
        p = Z[:, :, 0]
        if mode == 3:
            out = [mul(A0, p), 1j * mul(A1, p)]
        else:
            q = Z[:, :, 1]
            out = [mul(A0, p) - 1j * mul(A1, q)]
            if mode != 2:
                out.append(1j * mul(A1, p) + mul(A0, q))
        O = torch.stack(out, dim=2)                                                        # (., ., nout, Rp)
        return torch.stack([O.real, O.imag], dim=2).reshape(O.shape[0], O.shape[1], 2, -1).to(X.dtype).contiguous()

    @staticmethod
    def vcols_repack(src, dst, ncols, src_c0, dst_c0, zero_tail):
        dst[..., dst_c0:dst_c0 + ncols] = src[..., src_c0:src_c0 + ncols]
        if zero_tail and ncols > 0:                        # (the kernel launches nothing for zero columns)
            dst[..., dst_c0 + ncols:] = 0


def _s_to_complex(S, P, blocks):
    """S (L, M, 2, blocks / 2 * Rp) -> (blocks / 2, P, L, M) complex"""
    L, M = S.shape[:2]
    Sv = S.reshape(L, M, 2, blocks // 2, -1)[..., :P]
    return torch.complex(Sv[:, :, 0], Sv[:, :, 1]).permute(2, 3, 0, 1)


def _complex_to_s(c):
    """(nk, P, L, M) complex -> S (L, M, 2, nk * round32(P))"""
    nk, P, L, M = c.shape
    S = torch.stack([c.real, c.imag], dim=0).permute(3, 4, 0, 1, 2)                       # (L, M, 2, nk, P)
    return torch.nn.functional.pad(S, (0, _round32(P) - P)).reshape(L, M, 2, -1).contiguous()


def _dot(a, b):
    return (torch.view_as_real(a) * torch.view_as_real(b)).sum() if a.is_complex() else (a * b).sum()


def _close(a, b, what, rank):
    err = (a - b).abs().max().item() if a.numel() else 0.0
    bound = GATE * max(1.0, b.abs().max().item() if b.numel() else 0.0)
    assert err < bound, (rank, what, err, bound)


def _polar_exchanges(thd):
    return sum(v["all_to_alls"] for k, v in thd.COMM_STATS.items() if k[0] == "polar")


def _worker(rank, world, rendezvous, h, w, cases):
    torch.set_num_threads(1)
    with ranks(rank, world, rendezvous) as dist:
        import _vsht_ref as ref
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        from makani_amd import dist_pipeline as dp
        _, ih, iw = mcomm.init(h, w)
        assert thd.ensure_initialized()
        thd._BACKEND = VectorOracleBackend                      # test-only: the CPU stand-in for the HIP kernels
        for nlat, nlon, lmax, mmax, grid, P in cases:
            kw = dict(lmax=lmax, mmax=mmax, grid=grid)
            fwd = thd.DistributedRealVectorSHT(nlat, nlon, **kw)
            inv = thd.DistributedInverseRealVectorSHT(nlat, nlon, **kw)
            rfw = ref.RealVectorSHT(nlat, nlon, matrices=ref.library_matrices, **kw)
            riv = ref.InverseRealVectorSHT(nlat, nlon, matrices=ref.library_matrices, **kw)
            ll, ml, hl, wl = fwd.l_shapes[ih], fwd.m_shapes[iw], fwd.lat_shapes[ih], fwd.lon_shapes[iw]
            l0, m0, la0, lo0 = fwd.l_off, fwd.m_off, sum(fwd.lat_shapes[:ih]), sum(fwd.lon_shapes[:iw])
            assert fwd.weights.shape[:3] == (2, ml, lmax) and inv.pct_t.shape[:3] == (2, ml, nlat)          # the m-slice only
            assert fwd.band_lo is None or fwd.band_lo.shape == (ml,)
            spec = (Ellipsis, slice(l0, l0 + ll), slice(m0, m0 + ml))
            spat = (Ellipsis, slice(la0, la0 + hl), slice(lo0, lo0 + wl))
            tri = (torch.arange(lmax)[:, None] >= torch.arange(mmax)[None, :])[spec]
            gen = torch.Generator().manual_seed(100 * P + nlat)
            x = torch.randn(2, P, nlat, nlon, generator=gen, dtype=torch.float64)
            G = torch.complex(torch.randn(2, P, lmax, mmax, generator=gen, dtype=torch.float64),
                              torch.randn(2, P, lmax, mmax, generator=gen, dtype=torch.float64))
            coef = ref.lower_triangle(torch.complex(torch.randn(2, P, lmax, mmax, generator=gen, dtype=torch.float64),
                                                    torch.randn(2, P, lmax, mmax, generator=gen, dtype=torch.float64)))
            Gy = torch.randn(2, P, nlat, nlon, generator=gen, dtype=torch.float64)
            rf = lambda t: rfw(t.transpose(0, 1)).transpose(0, 1)                         # (2, P, ..) <-> the reference's (P, 2, ..)
            ri = lambda t: riv(t.transpose(0, 1)).transpose(0, 1)
            tag = f"h{h}w{w} {nlat}x{nlon} P={P}"
            dp.FALLBACKS.clear()

            # ---- analysis (modes 0 and, backward, 1) and its s-only form (modes 2 / 3) ----
            xs = x.clone().requires_grad_(True)
            cref = rf(xs)
            _dot(cref, G).backward()
            for s_only in (False, True):
                xl = x[spat].clone().requires_grad_(True)
                S = fwd.analysis(xl, s_only=s_only)
                nk = 1 if s_only else 2
                assert S.shape == (ll, ml, 2, nk * _round32(P)), (tag, S.shape)
                assert not S.reshape(ll, ml, 2 * nk, -1)[..., P:].any(), (tag, "pad columns must be zeros")
                c = _s_to_complex(S, P, 2 * nk)
                _close(c, cref.detach()[:nk][spec], f"{tag} analysis s_only={s_only}", rank)
                _dot(c, G[:nk][spec]).backward()
                if s_only:
                    xs2 = x.clone().requires_grad_(True)
                    _dot(rf(xs2)[:1], G[:1]).backward()
                    _close(xl.grad, xs2.grad[spat], f"{tag} analysis grad s_only", rank)
                else:
                    _close(xl.grad, xs.grad[spat], f"{tag} analysis grad", rank)

            # ---- synthesis (modes 1 / 0) and its t = 0 form (modes 3 / 2) ----
            for t_zero in (False, True):
                nk = 1 if t_zero else 2
                full = coef.clone()
                if t_zero:
                    full[1] = 0
                cs = full.clone().requires_grad_(True)
                yref = ri(cs)
                _dot(yref, Gy).backward()
                cl = full[:nk][spec].clone().requires_grad_(True)
                y = inv.synthesis(_complex_to_s(cl), P, out_dtype=torch.float64, t_zero=t_zero)
                assert y.shape == (2, P, hl, wl)
                _close(y, yref.detach()[spat], f"{tag} synthesis t_zero={t_zero}", rank)
                _dot(y, Gy[spat]).backward()
                _close(cl.grad * tri, cs.grad[:nk][spec] * tri, f"{tag} synthesis grad t_zero={t_zero}", rank)

            # ---- the chained round trip: Legendre-phase operand handed over, no polar exchange at all ----
            xs = x.clone().requires_grad_(True)
            bref = ri(rf(xs))
            _dot(bref, Gy).backward()
            xl = x[spat].clone().requires_grad_(True)
            before = _polar_exchanges(thd)
            T = fwd.analysis(xl, legendre_phase=True)
            ph = fwd._plane_shapes(P)[1][ih]
            assert T.shape == (lmax, ml, 2, 2 * _round32(ph)), (tag, T.shape)
            back = inv.synthesis(T, P, out_dtype=torch.float64, legendre_phase=True)
            _dot(back, Gy[spat]).backward()
            assert _polar_exchanges(thd) - before == (4 if h > 1 else 0), tag       # two forward, two backward (not four and four)
            _close(back, bref.detach()[spat], f"{tag} round trip", rank)
            _close(xl.grad, xs.grad[spat], f"{tag} round trip grad", rank)
            assert dp.FALLBACKS == [], "the vector pair has no fused form to fall back from"


CASES = [(33, 64, 33, 33, "equiangular", 3),       # poles on the grid, odd pair count
         (33, 64, 33, 33, "equiangular", 1),       # ranks that hold zero pairs in a phase still enter every collective
         (31, 64, 30, 24, "lobatto", 3)]           # ragged latitudes, l and m splits


def _run_layout(h, w):
    launch(_worker, h * w, h, w, CASES, limit=240)


def test_vector_schedule_matches_serial_h2w1():
    _run_layout(2, 1)


def test_vector_schedule_matches_serial_h1w2():
    _run_layout(1, 2)


def test_vector_schedule_matches_serial_h2w2():
    _run_layout(2, 2)


def test_vector_schedule_matches_serial_h3w2():
    _run_layout(3, 2)


# ---- contracts ---------------------------------------------------------------------------------------------------------------
def test_new_classes_and_entry_point_are_declared():
    import makani_amd as ma
    import makani_amd.distributed as thd
    from makani_amd.sht import RealVectorSHT, InverseRealVectorSHT
    assert ma.DistributedRealVectorSHT is thd.DistributedRealVectorSHT and "DistributedRealVectorSHT" in ma.__all__
    assert ma.DistributedInverseRealVectorSHT is thd.DistributedInverseRealVectorSHT and "DistributedInverseRealVectorSHT" in ma.__all__
    for cls, base in ((thd.DistributedRealVectorSHT, RealVectorSHT), (thd.DistributedInverseRealVectorSHT, InverseRealVectorSHT)):
        assert issubclass(cls, base) and issubclass(cls, thd._DistBase)
    assert hasattr(thd.HipBackend, "vlegendre") and hasattr(thd.HipBackend, "vcols_repack")


NAMES = ["u500", "v500", "u850", "v850", "t500"]


def _worker_losses(rank, world, rendezvous, h, w, n):
    torch.set_num_threads(1)
    with ranks(rank, world, rendezvous) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        _, ih, iw = mcomm.init(h, w, ensemble=n)
        assert mcomm.get_size("spatial") == h * w and mcomm.get_size("ensemble") == n
        kw = dict(img_shape=(17, 32), crop_shape=(17, 32), crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")
        for cls in (ma.GradientCRPSLoss, ma.VortDivCRPSLoss):
            loss = cls(spatial_distributed=True, ensemble_distributed=True, **kw)
            assert loss.spatial_distributed and loss.ensemble_distributed
            hl, wl = thd.compute_split_shapes(17, h)[ih], thd.compute_split_shapes(32, w)[iw]
            assert tuple(loss.quadrature.quad_weight.shape[-2:]) == (hl, wl)
            inv = loss.ivsht if cls is ma.GradientCRPSLoss else loss.isht
            fw = loss.sht if cls is ma.GradientCRPSLoss else loss.vsht
            assert isinstance(inv, thd.DistributedInverseRealVectorSHT)
            assert isinstance(fw, thd.DistributedRealSHT if cls is ma.GradientCRPSLoss else thd.DistributedRealVectorSHT)
            assert len(loss.state_dict()) == 0
            off = cls(**kw)                                                              # flags off: the serial modules on any tree
            assert not off.spatial_distributed and not off.ensemble_distributed and not isinstance(off.__dict__["_modules"][
                "ivsht" if cls is ma.GradientCRPSLoss else "isht"], thd.DistributedInverseRealVectorSHT)


def test_losses_construct_with_both_flags_on_a_real_tree():
    launch(_worker_losses, 4, 2, 1, 2, limit=240)
