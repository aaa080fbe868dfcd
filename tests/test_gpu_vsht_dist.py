"""GPU tests of the h x w distributed vector transform pair and of what it is built from: the m-shard form of the vector
Legendre launch (csrc/vlegendre.hip with tri_off and sliced matrices / bands), the column-block repack kernel of the pair-axis
exchanges (csrc/vcols.hip), the modules DistributedRealVectorSHT / DistributedInverseRealVectorSHT and the gradient / vort-div
CRPS losses on split groups.  The multi-rank tests are several processes sharing cuda:0 over gloo (host-staged exchanges) in
the pattern of tests/test_gpu_noise_dist.py; RCCL with more than one rank has not run this code."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _vsht_ref as ref
from _ranks import launch, ranks

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vsht_losses.npz")
TOL = 1e-5            # tests/test_gpu_vsht.py: three limbs; two limbs (allow_tf32) 2e-5


# ----------------------------------------------------------------------------------------------------------------------
# a. the m-shard form of mk_vlegendre through the C ABI
# ----------------------------------------------------------------------------------------------------------------------
def _vleg_call(mats, band, X, out, mode, limbs, rows, K, tri_off):
    from makani_amd import ops
    from makani_amd._lib import lib, ptr, check, stream
    p0, p1 = ops.limb_planes(mats[0]), ops.limb_planes(mats[1])
    lo, hi = band if band is not None else (None, None)
    orders, Rp = mats[0].shape[0], 64
    check(lib().mk_vlegendre(ptr(p0), ptr(p1), p0.stride(0), p0.stride(1), p0.stride(2), limbs, ptr(X), ptr(out), mode, rows, K,
                             orders, Rp, tri_off, ptr(lo), ptr(hi), stream()), "mk_vlegendre")
    return p0, p1                                   # (kept alive by the caller until the launch has run)


@pytest.mark.parametrize("band_on", [True, False])
def test_m_shard_launch_equals_the_order_slice_of_the_full_launch_bit_for_bit(band_on, monkeypatch):
    """orders [m0, m1) of a transform (nlat 64, L = M = 40, 35 pairs = two 32-column blocks) with tri_off = m0, sliced matrices and
    sliced bands against the same orders of the full launch: all four modes, two and three limbs.  The outputs are pre-filled with
    a sentinel, so the rows the triangle skips (never written) must be the same rows too."""
    import makani_amd as ma
    from makani_amd import ops
    monkeypatch.setattr(ops, "BAND_EPS", 1e-18 if band_on else 0.0)
    nlat, L, M, P = 64, 40, 40, 35
    Rp = ops.round32(P)
    fw = ma.RealVectorSHT(nlat, 128, lmax=L, mmax=M, grid="equiangular").to(DEV)
    assert (fw.band_lo is not None) == band_on
    if band_on:
        assert int(fw.band_lo.max()) > 0 and int(fw.band_hi.min()) < nlat           # the band does clip something
    gen = torch.Generator().manual_seed(21)
    tr = (fw.weights_t[0], fw.weights_t[1])                       # (M, nlat, lp): analysis-shaped launches (modes 0, 2)
    nat = (fw.weights[0], fw.weights[1])                          # (M, L, kp): synthesis-shaped launches (modes 1, 3)
    for mode in range(4):
        ana = mode in (0, 2)
        nib, nob = (2 if mode == 3 else 4), (2 if mode == 2 else 4)
        mats, rows, K = (tr, L, nlat) if ana else (nat, nlat, L)
        X = torch.randn((M, nlat, nib * Rp) if ana else (L, M, nib * Rp), generator=gen).to(DEV)
        for limbs in (3, 2):
            full = torch.full((L, M, nob * Rp) if ana else (M, nlat, nob * Rp), 7.0, device=DEV)
            band = (fw.band_lo, fw.band_hi) if band_on else None
            keep = [_vleg_call(mats, band, X, full, mode, limbs, rows, K, 0)]
            torch.cuda.synchronize()
            assert torch.isfinite(full).all() and bool((full != 7.0).any())
            for m0, m1 in ((0, 20), (20, 40), (17, 33)):
                ms = tuple(t[m0:m1].contiguous() for t in mats)
                bs = (fw.band_lo[m0:m1].contiguous(), fw.band_hi[m0:m1].contiguous()) if band_on else None
                Xs = (X[m0:m1] if ana else X[:, m0:m1]).contiguous()
                out = torch.full((L, m1 - m0, nob * Rp) if ana else (m1 - m0, nlat, nob * Rp), 7.0, device=DEV)
                keep.append((ms, bs, _vleg_call(ms, bs, Xs, out, mode, limbs, rows, K, m0)))
                want = full[:, m0:m1] if ana else full[m0:m1]
                same = torch.equal(out, want)
                print(f"mode {mode} limbs {limbs} band {band_on} orders [{m0}, {m1}): bit-equal {same}, "
                      f"max |diff| {float((out - want).abs().max()):.2e}")
                assert same, (mode, limbs, m0, m1)


# ----------------------------------------------------------------------------------------------------------------------
# b. the repack kernel against the torch indexing expression
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [2, 4])
@pytest.mark.parametrize("ncols,src_c0,dst_c0,src_rp,dst_rp", [
    (7, 3, 5, 32, 64),          # nothing aligned: 4-byte accesses
    (5, 0, 0, 5, 32),           # an arriving slab without padding into the padded operand (unpack)
    (3, 29, 0, 32, 3),          # the last columns of a block into a slab without padding (pack)
    (8, 4, 12, 32, 32),         # everything a multiple of 4: 16-byte accesses
    (32, 32, 0, 64, 32),        # whole 32-column blocks
    (0, 0, 0, 32, 32),          # no columns: no launch, nothing written
])
def test_repack_kernel_equals_the_indexing_expression(blocks, ncols, src_c0, dst_c0, src_rp, dst_rp):
    from makani_amd import ops
    gen = torch.Generator().manual_seed(22)
    outer, inner = 5, 37
    for zero_tail in (False, True):
        for lat_range in (False, True):          # the destination rows are a latitude range of a larger tensor (an inner axis)
            src = torch.randn(outer, inner, blocks, src_rp, generator=gen).to(DEV)
            big = torch.full((outer, inner + 9 if lat_range else inner, blocks, dst_rp), float("nan"), device=DEV)
            dst = big.narrow(1, 4, inner) if lat_range else big
            want = big.clone()
            wv = want.narrow(1, 4, inner) if lat_range else want
            wv[..., dst_c0:dst_c0 + ncols] = src[..., src_c0:src_c0 + ncols]
            if zero_tail and ncols > 0:
                wv[..., dst_c0 + ncols:] = 0.0
            ops.vcols_repack(src, dst, ncols, src_c0, dst_c0, zero_tail)
            # NaN pre-fill: columns outside [dst_c0, dst_rp) (and everything without zero_tail beyond the copy) stay NaN, the
            # pad columns come back as exact zeros
            assert torch.equal(torch.isnan(big), torch.isnan(want))
            assert torch.equal(torch.nan_to_num(big, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), (zero_tail, lat_range)
            if zero_tail and ncols > 0:
                assert not big.narrow(1, 4, inner)[..., dst_c0 + ncols:].any() if lat_range else not big[..., dst_c0 + ncols:].any()
    # a source that is a row range of a larger tensor (the pack side of the lat <-> pairs exchange), more than one workgroup
    src_big = torch.randn(6, 50, blocks, 64, generator=gen).to(DEV)
    out = torch.full((6, 21, blocks, 12), float("nan"), device=DEV)
    ops.vcols_repack(src_big.narrow(1, 17, 21), out, 12, 40, 0, False)
    assert torch.equal(out, src_big[:, 17:38, :, 40:52])


# ----------------------------------------------------------------------------------------------------------------------
# d. the modules on split spheres against the fp64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def _global_rel(a, b):
    """rel-L2 of the gathered result: the ranks' shards of ``a`` against their shards of the reference ``b``"""
    a = a.detach().cpu()
    a = a.to(torch.complex128 if a.is_complex() else torch.float64)
    s = torch.stack([(a - b.to(a.dtype)).abs().pow(2).sum(), b.abs().pow(2).sum()]).double()
    dist.all_reduce(s)
    return math.sqrt(float(s[0]) / max(float(s[1]), 1e-300))


GRIDS = [(33, 64, 33, 33, "equiangular", 3),          # poles on the grid, odd pair count
         (33, 64, 33, 33, "equiangular", 1),          # ranks that hold no pair in a phase launch nothing and enter every collective
         (31, 64, 30, 24, "lobatto", 35)]             # ragged latitudes, truncated orders, more than one 32-column block


def _worker_modules(rank, world, rendezvous, h, w, bf16):
    with ranks(rank, world, rendezvous):
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        from makani_amd import ops
        dev = torch.device("cuda:0")
        _, ih, iw = mcomm.init(h, w)
        assert thd.ensure_initialized()
        for nlat, nlon, lmax, mmax, grid, P in GRIDS:
            kw = dict(lmax=lmax, mmax=mmax, grid=grid)
            fw, iv = ma.DistributedRealVectorSHT(nlat, nlon, **kw).to(dev), ma.DistributedInverseRealVectorSHT(nlat, nlon, **kw).to(dev)
            sfw, siv = ma.RealVectorSHT(nlat, nlon, **kw).to(dev), ma.InverseRealVectorSHT(nlat, nlon, **kw).to(dev)
            rfw = ref.RealVectorSHT(nlat, nlon, matrices=ref.library_matrices, **kw)
            riv = ref.InverseRealVectorSHT(nlat, nlon, matrices=ref.library_matrices, **kw)
            ll, ml, hl, wl = fw.l_shapes[ih], fw.m_shapes[iw], fw.lat_shapes[ih], fw.lon_shapes[iw]
            spec = (Ellipsis, slice(fw.l_off, fw.l_off + ll), slice(fw.m_off, fw.m_off + ml))
            la0, lo0 = sum(fw.lat_shapes[:ih]), sum(fw.lon_shapes[:iw])
            spat = (Ellipsis, slice(la0, la0 + hl), slice(lo0, lo0 + wl))
            tri_all = torch.arange(lmax)[:, None] >= torch.arange(mmax)[None, :]          # (the l < m entries never enter a transform)
            tri = tri_all[spec]
            gen = torch.Generator().manual_seed(31 + P)
            x = torch.randn(P, 2, nlat, nlon, generator=gen)
            ct = ref.lower_triangle(torch.complex(torch.randn(P, 2, lmax, mmax, generator=gen), torch.randn(P, 2, lmax, mmax, generator=gen)))
            c = ref.lower_triangle(torch.complex(torch.randn(P, 2, lmax, mmax, generator=gen), torch.randn(P, 2, lmax, mmax, generator=gen)))
            cx = torch.randn(P, 2, nlat, nlon, generator=gen)
            xr = x.double().requires_grad_(True)
            yr = rfw(xr)
            (gxr,) = torch.autograd.grad(yr, xr, ct.to(torch.complex128))
            cr = c.to(torch.complex128).requires_grad_(True)
            zr = riv(cr)
            (gcr,) = torch.autograd.grad(zr, cr, cx.double())
            for tf32, tol in ((False, TOL), (True, 2e-5)):
                torch.backends.cuda.matmul.allow_tf32 = tf32
                assert ops.gemm_mode() == ("x3" if tf32 else "x6")
                xl = x[spat].to(dev).requires_grad_(True)
                y = fw(xl)
                assert y.shape == (P, 2, ll, ml) and y.dtype == torch.complex64
                (gx,) = torch.autograd.grad(y, xl, ct[spec].to(dev))
                cl = c[spec].to(dev).requires_grad_(True)
                z = iv(cl)
                assert z.shape == (P, 2, hl, wl) and z.dtype == torch.float32
                (gc,) = torch.autograd.grad(z, cl, cx[spat].to(dev))
                e = [_global_rel(y, yr.detach()[spec]), _global_rel(gx, gxr[spat]), _global_rel(z, zr.detach()[spat]),
                     _global_rel(gc.cpu() * tri, (gcr * tri_all)[spec])]
                with torch.no_grad():
                    ds = [_global_rel(y, sfw(x.to(dev)).cpu()[spec]), _global_rel(z, siv(c.to(dev)).cpu()[spat])]
                if rank == 0:
                    print(f"h{h}w{w} {nlat}x{nlon} P={P} {'two' if tf32 else 'three'} limbs: fwd {e[0]:.2e} fwd-grad {e[1]:.2e} inv {e[2]:.2e} "
                          f"inv-grad {e[3]:.2e}; to the serial HIP modules: fwd {ds[0]:.2e} inv {ds[1]:.2e}", flush=True)
                assert max(e) <= tol, (rank, h, w, nlat, P, tf32, e)
            if bf16:
                torch.backends.cuda.matmul.allow_tf32 = False
                xb = x.bfloat16()
                yb = fw(xb[spat].to(dev))
                eb = _global_rel(yb, rfw(xb.double())[spec])
                if rank == 0:
                    print(f"h{h}w{w} {nlat}x{nlon} P={P} bf16 input: fwd {eb:.2e}", flush=True)
                assert yb.dtype == torch.complex64 and eb <= TOL, (rank, eb)


@pytest.mark.parametrize("h,w,bf16", [(2, 2, True), (1, 2, False), (3, 1, False)])
def test_distributed_vector_modules_match_fp64(h, w, bf16):
    launch(_worker_modules, h * w, h, w, bf16, limit=240)


# ----------------------------------------------------------------------------------------------------------------------
# e. the two losses on split groups against the fixtures recorded from the reference's own classes
# ----------------------------------------------------------------------------------------------------------------------
def _worker_losses(rank, world, rendezvous, h, w, n):
    with ranks(rank, world, rendezvous):
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        dev = torch.device("cuda:0")
        torch.backends.cuda.matmul.allow_tf32 = False
        _, ih, iw = mcomm.init(h, w, ensemble=n)
        ie = mcomm.get_rank("ensemble")
        assert thd.ensure_initialized() and mcomm.get_size("ensemble") == n
        z = np.load(GOLDEN)
        ran = 0
        for case in sorted({k.split("/")[0] for k in z.files}):
            meta = json.loads(str(z[f"{case}/meta"]))
            f = torch.from_numpy(z[f"{case}/forecasts"])
            E = f.shape[1]
            if E % n:
                continue                                   # (the ensemble layout takes the cases whose member count splits evenly)
            ran += 1
            loss = getattr(ma, meta["cls"])(spatial_distributed=True, ensemble_distributed=n > 1, **meta["kwargs"]).to(dev)
            assert loss.spatial_distributed and loss.ensemble_distributed == (n > 1)
            H, W = f.shape[-2:]
            lat, lon = thd.compute_split_shapes(H, h), thd.compute_split_shapes(W, w)
            spat = (Ellipsis, slice(sum(lat[:ih]), sum(lat[:ih + 1])), slice(sum(lon[:iw]), sum(lon[:iw + 1])))
            mem = slice(ie * (E // n), (ie + 1) * (E // n))
            fl = f[:, mem][spat].to(dev).requires_grad_(True)
            o = torch.from_numpy(z[f"{case}/observations"])[spat].to(dev)
            wgt = torch.from_numpy(z[f"{case}/weights"])[spat].to(dev) if f"{case}/weights" in z.files else None
            out = loss(fl, o, wgt)
            want = torch.from_numpy(z[f"{case}/out"])
            assert out.shape == want.shape
            (gf,) = torch.autograd.grad(out.sum(), fl)
            ev = ref.rel_l2(out, want)
            eg = _global_rel(gf, torch.from_numpy(z[f"{case}/grad"])[:, mem][spat])
            if rank == 0:
                print(f"h{h}w{w} x ensemble {n} {case}{' (spatial weights)' if wgt is not None else ''}: value {ev:.2e} gradient {eg:.2e}", flush=True)
            assert ev <= 1e-5 and eg <= 1e-5, (rank, case, ev, eg)
        assert ran >= 2


@pytest.mark.parametrize("h,w,n", [(2, 2, 1), (2, 1, 2)])
def test_losses_on_split_groups_match_the_reference_fixtures(h, w, n):
    """every recorded case scattered over h2 w2, and the cases with an even member count over h2 w1 x ensemble 2: loss value and
    gathered forecast gradient within 1e-5, the gate of test_losses_match_the_reference_fixtures (same fixtures)"""
    assert os.path.exists(GOLDEN)
    launch(_worker_losses, h * w * n, h, w, n, limit=240)


# ----------------------------------------------------------------------------------------------------------------------
# f. graph replay of the exchange path with groups of one rank
# ----------------------------------------------------------------------------------------------------------------------
def _worker_graph(rank, world, rendezvous):
    with ranks(rank, world, rendezvous):
        import makani_amd as ma
        import makani_amd.distributed as thd
        dev = torch.device("cuda:0")
        g = dist.new_group([0])
        thd.init(g, g, g)                    # groups of ONE rank: every pack / unpack launch runs, nothing leaves the device
        fw = ma.DistributedRealVectorSHT(33, 64, grid="equiangular").to(dev)
        iv = ma.DistributedInverseRealVectorSHT(33, 64, grid="equiangular").to(dev)
        sfw, siv = ma.RealVectorSHT(33, 64, grid="equiangular").to(dev), ma.InverseRealVectorSHT(33, 64, grid="equiangular").to(dev)
        x = torch.randn(3, 2, 33, 64, device=dev)
        calls = []
        real = thd.HipBackend.vcols_repack
        thd.HipBackend.vcols_repack = staticmethod(lambda *a: (calls.append(1), real(*a))[1])
        eager = iv(fw(x))                    # also warms up plans, limb planes and bands outside the capture
        thd.HipBackend.vcols_repack = staticmethod(real)
        assert len(calls) == 6, calls        # per transform three exchanges on the column blocks, one pass each (the own share)
        serial = siv(sfw(x))
        print(f"one-rank groups against the serial pair: max |diff| {float((eager - serial).abs().max()):.2e}", flush=True)
        assert torch.equal(eager, serial)    # the same launches on the same values: the repack passes only move them
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                out = iv(fw(x))
        torch.cuda.current_stream().wait_stream(stream)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_exchange_path_replays_from_a_captured_graph():
    launch(_worker_graph, 1, limit=240)
