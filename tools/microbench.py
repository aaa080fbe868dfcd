"""Per-kernel microbenchmarks at the BASELINE shapes (HIP events on the launch stream).
   python tools/microbench.py [fft] [legendre] [dhconv] [pointwise] [vsht] [escore] [noise] [noise_shard] [losses] [coherence] [metrics] [preproc] [constraints] [interpolant] [losshandler] [mhandler] [fcn31]"""
import os, sys, time, math, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from makani_amd import ops
import makani_amd as ma

dev = torch.device("cuda:0")


def timeit(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fft():
    C = 384
    for nlat, nlon, mmax in ((721, 1440, 241), (240, 480, 241)):
        c = 2 * math.pi / nlon
        for dt in (torch.float32, torch.bfloat16):
            x = torch.rand(1, C, nlat, nlon, device=dev).to(dt)
            ms = timeit(lambda: ops.rfft_rows(x, mmax, C, (c, c, c)))
            nb = C * nlat * (nlon * x.element_size() + mmax * 8)
            print(f"rfft  {nlat}x{nlon} {str(dt)[6:]:9s} {ms:8.3f} ms  {nb/ms/1e6:8.1f} GB/s  ({nb/1e6:.0f} MB)")
            F = ops.rfft_rows(x, mmax, C, (c, c, c))
            ms = timeit(lambda: ops.irfft_rows(F, 1, C, nlon, dt, (1.0, 2.0, 1.0)))
            print(f"irfft {nlat}x{nlon} {str(dt)[6:]:9s} {ms:8.3f} ms  {nb/ms/1e6:8.1f} GB/s")
            del x, F


def legendre():
    C = 384
    for nlat, nlon, grid in ((721, 1440, "equiangular"), (240, 480, "legendre-gauss")):
        S = ma.RealSHT(nlat, nlon, lmax=240, mmax=241, grid=grid).to(dev)
        I = ma.InverseRealSHT(nlat, nlon, lmax=240, mmax=241, grid=grid).to(dev)
        F = torch.randn(241, nlat, 2, C, device=dev)
        Sc = torch.randn(240, 241, 2, C, device=dev)
        fl = 4.0 * C * nlat * 240 * 241

        def run(gen):
            a = ops.legendre_analysis(F, S.weights_t, 240)
            b = ops.legendre_synthesis(Sc, I.pct, nlat)
            ms = timeit(lambda: ops.legendre_analysis(F, S.weights_t, 240))
            print(f"gen{gen} analysis  K={nlat}: {ms:7.3f} ms  {fl/ms/1e9:7.1f} TF dense-equiv")
            ms = timeit(lambda: ops.legendre_synthesis(Sc, I.pct, nlat))
            print(f"gen{gen} synthesis K={nlat}: {ms:7.3f} ms  {fl/ms/1e9:7.1f} TF dense-equiv")
            return a, b
        run("2")


def dhconv():
    C, L, M = 384, 240, 241
    S = torch.randn(L, M, 2, C, device=dev)
    G = torch.randn(L, M, 2, C, device=dev)
    w = ops.native_w_empty(C, C, L, dev)
    w.copy_(torch.randn(1, C, C, L, dtype=torch.complex64, device=dev))
    fl = 8.0 * C * C * L * M
    tri = (torch.arange(L, device=dev)[:, None] >= torch.arange(M, device=dev)[None, :])[:, :, None, None]

    def run(gen):
        y = ops.dhconv_fwd(S, w, 1, C)
        gs = ops.dhconv_dgrad(G, w, 1, C, C)
        gw = ops.dhconv_wgrad(S, G, 1, native=True)
        ms = timeit(lambda: ops.dhconv_fwd(S, w, 1, C)); print(f"gen{gen} dhconv fwd  : {ms:7.3f} ms {fl/ms/1e9:7.1f} TF dense-equiv")
        ms = timeit(lambda: ops.dhconv_dgrad(G, w, 1, C, C)); print(f"gen{gen} dhconv dgrad: {ms:7.3f} ms {fl/ms/1e9:7.1f} TF dense-equiv")
        ms = timeit(lambda: ops.dhconv_wgrad(S, G, 1, native=True)); print(f"gen{gen} dhconv wgrad: {ms:7.3f} ms {fl/ms/1e9:7.1f} TF dense-equiv")
        return y, gs, torch.view_as_real(gw)
    run("2")


def pointwise():
    for H, W in ((240, 480), (721, 1440)):
        x = torch.randn(1, 384, H, W, device=dev).bfloat16().requires_grad_(True)
        g = torch.ones(384, device=dev); b = torch.zeros(384, device=dev)
        nb = x.numel() * 2
        for gelu in (False, True):
            tag = "instnorm+gelu" if gelu else "instnorm     "
            ms = timeit(lambda: ops.InstanceNormFn.apply(x, g, b, 1e-6, gelu))
            print(f"{tag} fwd {H}x{W}: {ms:7.3f} ms  {3*nb/ms/1e6:7.1f} GB/s (2 reads + 1 write)")
            y = ops.InstanceNormFn.apply(x, g, b, 1e-6, gelu)
            gy = torch.randn_like(y)
            ms = timeit(lambda: torch.autograd.grad(y, x, gy, retain_graph=True))
            print(f"{tag} bwd {H}x{W}: {ms:7.3f} ms  {5*nb/ms/1e6:7.1f} GB/s (4 reads + 1 write)")
        ms = timeit(lambda: ops.BiasGeluFn.apply(x, b))
        print(f"bias_gelu fwd     {H}x{W}: {ms:7.3f} ms  {2*nb/ms/1e6:7.1f} GB/s")


def cold():
    """streaming kernels on ROTATING buffers (12 x 88 MB inputs: nothing is left in the 256 MB memory-side cache or
    the L2s from the previous call) — what the kernels see inside the train step"""
    NB, C, H, W = 12, 384, 240, 480
    xs = [torch.randn(1, C, H, W, device=dev).bfloat16() for _ in range(NB)]
    ys = [torch.empty_like(x) for x in xs]
    g = torch.ones(C, device=dev); b = torch.zeros(C, device=dev)
    nb = xs[0].numel() * 2
    it = [0]
    def rot(fn):
        def f():
            i = it[0] = (it[0] + 1) % NB
            fn(i)
        return f
    ms = timeit(rot(lambda i: torch.add(xs[i], xs[(i + 5) % NB], out=ys[i])), reps=24, warm=12)
    print(f"cold torch add bf16       : {ms*1e3:7.1f} us  {3*nb/ms/1e6:7.1f} GB/s")
    ms = timeit(rot(lambda i: ys[i].copy_(xs[i])), reps=24, warm=12)
    print(f"cold torch copy bf16      : {ms*1e3:7.1f} us  {2*nb/ms/1e6:7.1f} GB/s")
    ms = timeit(rot(lambda i: ops._sum_planes(xs[i])), reps=24, warm=12)
    print(f"cold plane sums           : {ms*1e3:7.1f} us  {nb/ms/1e6:7.1f} GB/s")
    ms = timeit(rot(lambda i: xs[i].sum(dim=(0, 2, 3), dtype=torch.float32)), reps=24, warm=12)
    print(f"cold torch sum(0,2,3)     : {ms*1e3:7.1f} us  {nb/ms/1e6:7.1f} GB/s")
    for gelu in (False, True):
        ms = timeit(rot(lambda i: ops.InstanceNormFn.apply(xs[i], g, b, 1e-6, gelu)), reps=24, warm=12)
        print(f"cold instnorm fwd gelu={int(gelu)}  : {ms*1e3:7.1f} us  {3*nb/ms/1e6:7.1f} GB/s (2 reads + 1 write)")
    pbias = torch.randn(C, device=dev) * 0.1
    ms = timeit(rot(lambda i: ops.InstanceNormFn.apply(xs[i], g, b, 1e-6, False, pbias)), reps=24, warm=12)
    print(f"cold instnorm fwd pre_bias: {ms*1e3:7.1f} us  {3*nb/ms/1e6:7.1f} GB/s (2 reads + 1 write)")
    xr = [x.clone().requires_grad_(True) for x in xs]
    outs = [ops.InstanceNormFn.apply(x, g, b, 1e-6, False, pbias) for x in xr]
    ms = timeit(rot(lambda i: torch.autograd.grad(outs[i], xr[i], ys[i], retain_graph=True)), reps=24, warm=12)
    print(f"cold instnorm bwd pre_bias: {ms*1e3:7.1f} us  {5*nb/ms/1e6:7.1f} GB/s (4 reads + 1 write)")
    del outs
    for gelu in (False, True):
        outs = [ops.InstanceNormFn.apply(x, g, b, 1e-6, gelu) for x in xr]
        ms = timeit(rot(lambda i: torch.autograd.grad(outs[i], xr[i], ys[i], retain_graph=True)), reps=24, warm=12)
        print(f"cold instnorm bwd gelu={int(gelu)}  : {ms*1e3:7.1f} us  {5*nb/ms/1e6:7.1f} GB/s (4 reads + 1 write)")
        del outs
    c = 2 * math.pi / W
    Fs = [ops.rfft_rows(xs[i], 241, C, (c, c, c)) for i in range(NB)]
    nbf = C * H * (W * 2 + 241 * 8)
    ms = timeit(rot(lambda i: ops.rfft_rows(xs[i], 241, C, (c, c, c))), reps=24, warm=12)
    print(f"cold rfft 240x480 bf16    : {ms*1e3:7.1f} us  {nbf/ms/1e6:7.1f} GB/s")
    ms = timeit(rot(lambda i: ops.irfft_rows(Fs[i], 1, C, W, torch.bfloat16, (1.0, 2.0, 1.0))), reps=24, warm=12)
    print(f"cold irfft 240x480 bf16   : {ms*1e3:7.1f} us  {nbf/ms/1e6:7.1f} GB/s")
    ms = timeit(lambda: ops.rfft_rows(xs[0], 241, C, (c, c, c)), reps=24, warm=4)
    print(f"warm rfft 240x480 bf16    : {ms*1e3:7.1f} us  {nbf/ms/1e6:7.1f} GB/s")
    ms = timeit(lambda: ops.irfft_rows(Fs[0], 1, C, W, torch.bfloat16, (1.0, 2.0, 1.0)), reps=24, warm=4)
    print(f"warm irfft 240x480 bf16   : {ms*1e3:7.1f} us  {nbf/ms/1e6:7.1f} GB/s")


def conv():
    """forward / data-gradient channel GEMM: HIP kernel against the library GEMM, plain and with the fused epilogues; each
    result checked against fp32"""
    per_step = {(768, 384, 721): 2, (384, 768, 721): 2, (384, 384, 721): 8, (768, 384, 240): 14, (384, 768, 240): 14, (384, 384, 240): 14}
    tot_hip = tot_lib = 0.0
    for (M, K, H, W) in ((768, 384, 721, 1440), (384, 768, 721, 1440), (384, 384, 721, 1440), (768, 384, 240, 480),
                         (384, 768, 240, 480), (384, 384, 240, 480), (73, 384, 721, 1440), (384, 73, 721, 1440)):
        torch.manual_seed(M + K)
        x = (torch.rand(1, K, H, W, device=dev) - 0.5).bfloat16()
        w = (torch.randn(M, K, device=dev) / K ** 0.5).bfloat16()
        bias = torch.randn(M, device=dev)
        A = ops.pad_weight_bf16(w)
        fl = 2.0 * M * K * H * W
        nb = 2.0 * H * W * (M + K)
        ref = torch.mm(w.float(), x.view(K, -1).float())
        y, _ = ops.conv1x1_nn(A, K, x)
        err = ((y.view(M, -1).float() - ref).norm() / ref.norm()).item()
        gsrc = torch.randn(1, M, H, W, device=dev).bfloat16()
        res = torch.randn(1, M, H, W, device=dev).bfloat16()
        y2, pre = ops.conv1x1_nn(A, K, x, bias=bias, act=True, want_pre=True, residual=res)
        pre_ref = (ref + bias[:, None]).bfloat16().float()
        ref2 = torch.nn.functional.gelu(pre_ref) + res.view(M, -1).float()
        err2 = ((y2.view(M, -1).float() - ref2).norm() / ref2.norm()).item()
        errp = ((pre.view(M, -1).float() - pre_ref).norm() / pre_ref.norm()).item()
        del ref2, pre_ref, y2, pre
        ms = timeit(lambda: ops.conv1x1_nn(A, K, x), reps=20, warm=3)
        ms_b = timeit(lambda: ops.conv1x1_nn(A, K, x, bias=bias, act=True, want_pre=True), reps=20, warm=3)
        ms_g = timeit(lambda: ops.conv1x1_nn(A, K, x, gelu_grad_of=gsrc), reps=20, warm=3)
        ms_r = timeit(lambda: ops.conv1x1_nn(A, K, x, residual=res), reps=20, warm=3)
        out = torch.empty(M, H * W, device=dev, dtype=torch.bfloat16)
        ms2 = timeit(lambda: torch.mm(w, x.view(K, H * W), out=out), reps=20, warm=3)
        n = per_step.get((M, K, H), 0)
        tot_hip += n * ms
        tot_lib += n * ms2
        print(f"conv M={M:3d} K={K:3d} {H}x{W}: hip {ms:7.3f} ms ({fl/ms/1e9:5.0f} TF, {nb/ms/1e6:5.0f} GB/s) | lib {ms2:7.3f} ms ({fl/ms2/1e9:5.0f} TF)"
              f" | +bias+gelu+pre {ms_b:6.3f}  *gelu'(G) {ms_g:6.3f}  +R {ms_r:6.3f} | rel err {err:.1e} fused {err2:.1e} pre {errp:.1e}")
        del x, gsrc, res, ref, out
    print(f"fwd+dgrad GEMMs of the step at these shapes: hip {tot_hip:.2f} ms, library {tot_lib:.2f} ms")


def wgrad():
    """channel-GEMM weight gradient: the nine shapes of the train step (+ ragged / batched ones), checked against an fp32
    GEMM of the same bf16 operands, then timed."""
    shapes = [(768, 384, 1, 721, 1440), (384, 768, 1, 721, 1440), (384, 384, 1, 721, 1440), (384, 73, 1, 721, 1440),
              (73, 384, 1, 721, 1440), (73, 73, 1, 721, 1440), (768, 384, 1, 240, 480), (384, 768, 1, 240, 480),
              (384, 384, 1, 240, 480), (384, 200, 2, 91, 184), (300, 384, 1, 37, 72), (768, 384, 2, 60, 124)]
    per_step = {(768, 384, 721): 1, (384, 768, 721): 1, (384, 384, 721): 3, (384, 73, 721): 1, (73, 384, 721): 1, (73, 73, 721): 1,
                (768, 384, 240): 7, (384, 768, 240): 7, (384, 384, 240): 7}
    total = 0.0
    for (M, K, B, H, W) in shapes:
        torch.manual_seed(M + K + H)
        x = (torch.rand(B, K, H, W, device=dev) - 0.3).bfloat16()
        g = (torch.randn(B, M, H, W, device=dev) * 0.5).bfloat16()
        dW = ops.conv1x1_wgrad(g, x)
        ref = torch.einsum("bmn,bkn->mk", g.view(B, M, -1).float(), x.view(B, K, -1).float())
        err = ((dW - ref).norm() / ref.norm()).item()
        ms = timeit(lambda: ops.conv1x1_wgrad(g, x), reps=20, warm=3)
        nb = 2.0 * B * H * W * (M + K)
        n = per_step.get((M, K, H), 0)
        total += n * ms
        print(f"wgrad M={M:3d} K={K:3d} B={B} {H}x{W}: {ms:7.3f} ms  {nb/ms/1e6:7.0f} GB/s  {2.0*B*M*K*H*W/ms/1e9:6.0f} TF  rel err {err:.1e}"
              f"  {'x%d per step' % n if n else ''}")
        del x, g
    print(f"wgrad per step (29 launches): {total:.3f} ms  -> {16.72e3/total/1e3:.2f} TB/s algorithmic = {16.72e3/total/8e3:.3f} of 8 TB/s")


def spectral():
    """the HBM-streaming contractions (csrc/spectral_pointwise.hip): algorithmic bytes = activations in + out + weights once"""
    L, M = 240, 241
    for C in (64, 128):                       # diagonal: one C x C complex matrix per (l, m); 1.9 / 7.6 GB of weights
        S = torch.randn(L, M, 2, C, device=dev)
        w = torch.randn(1, C, C, L, M, dtype=torch.complex64, device=dev)
        wr = torch.view_as_real(w)
        T = torch.empty_like(S)
        gw = torch.empty_like(wr)
        nb = 8.0 * C * C * L * M + 2 * 8.0 * C * L * M
        live = 0.5 * 8.0 * C * C * L * M + 2 * 8.0 * C * L * M          # the l < m half of the weights is never read
        ms = timeit(lambda: ops.check(ops.lib().mk_spec_diag_apply(ops.ptr(S), ops.ptr(wr), ops.ptr(T), L, M, 1, C, C, C, C, 0, 0, 0, ops.stream())))
        print(f"diag fwd   C={C:3d}: {ms:7.3f} ms  {nb/ms/1e6:7.1f} GB/s dense  ({live/ms/1e6:7.1f} GB/s touched)")
        ms = timeit(lambda: ops.check(ops.lib().mk_spec_diag_apply(ops.ptr(S), ops.ptr(wr), ops.ptr(T), L, M, 1, C, C, C, C, 0, 0, 1, ops.stream())))
        print(f"diag dgrad C={C:3d}: {ms:7.3f} ms  {nb/ms/1e6:7.1f} GB/s dense  ({live/ms/1e6:7.1f} GB/s touched)")
        ms = timeit(lambda: ops.check(ops.lib().mk_spec_diag_wgrad(ops.ptr(S), ops.ptr(T), ops.ptr(gw), L, M, 1, C, C, C, C, 0, ops.stream())))
        print(f"diag wgrad C={C:3d}: {ms:7.3f} ms  {nb/ms/1e6:7.1f} GB/s (gradient written in full)")
        del S, w, wr, T, gw
    C = 384
    S = torch.randn(L, M, 2, C, device=dev)
    T = torch.empty_like(S)
    for Mw in (M, 1):
        Ws = torch.randn(L, Mw, 2, C, device=dev)
        gW = torch.empty_like(Ws)
        nb = 4.0 * (4 * C * L * M + 2 * C * L * Mw)
        ms = timeit(lambda: ops.check(ops.lib().mk_spec_sep_mul(ops.ptr(S), ops.ptr(Ws), ops.ptr(T), L, M, Mw, 1, C, 0, 0, ops.stream())))
        print(f"sep mul   Mw={Mw:3d}: {ms:7.3f} ms  {nb/ms/1e6:7.1f} GB/s dense")
        ms = timeit(lambda: ops.check(ops.lib().mk_spec_sep_wgrad(ops.ptr(S), ops.ptr(T), ops.ptr(gW), L, M, Mw, 1, C, 0, ops.stream())))
        print(f"sep wgrad Mw={Mw:3d}: {ms:7.3f} ms  {nb/ms/1e6:7.1f} GB/s dense")


def sht():
    """BASELINE's secondary metric "fwd SHT GB/s" (bench.py: sht_bandwidth): S1 ERA5-shaped (73 channels, full band),
    S2 model-shaped; plus the Legendre step of S1 alone (the narrow-operand form of the real split kernel, csrc/xgemm2.hip)"""
    for name, C, lmax, mmax in (("S1_c73_L721_M721", 73, 721, 721), ("S2_c384_L240_M241", 384, 240, 241)):
        S = ma.RealSHT(721, 1440, lmax=lmax, mmax=mmax, grid="equiangular").to(dev)
        x = torch.rand(1, C, 721, 1440, device=dev)
        ms = timeit(lambda: S(x), reps=10, warm=2)
        nb = C * 721 * 1440 * 4 + C * lmax * mmax * 8
        print(f"fwd SHT {name}: {ms:7.3f} ms  {nb/ms/1e6:7.1f} GB/s")
        if C == 73:
            R = ops.round4(C)
            F = torch.randn(mmax, 721, 2, R, device=dev)
            fl = 4.0 * C * 721 * lmax * mmax
            ms = timeit(lambda: ops.legendre_analysis(F, S.weights_t, lmax), reps=10, warm=2)
            print(f"   legendre analysis  C=73 full band: {ms:7.3f} ms  {fl/ms/1e9:7.1f} TF dense-equiv")
            c = 2 * math.pi / 1440
            ms = timeit(lambda: ops.rfft_rows(x, mmax, R, (c, c, c)), reps=10, warm=2)
            print(f"   rfft 1440 fp32 C=73 full spectrum : {ms:7.3f} ms")
        del S, x


def vsht():
    """vector Legendre stage (csrc/vlegendre.hip) for P pairs beside the SCALAR Legendre launch on 2 P planes (same F / S
    bytes, half the matrix bytes, half the MFMA work), same process, full band L = M = nlat; ratio = vector / scalar"""
    for nlat, nlon, grid, P in ((721, 1440, "equiangular", 64), (360, 720, "equiangular", 64)):
        L = M = nlat
        V = ma.RealVectorSHT(nlat, nlon, lmax=L, mmax=M, grid=grid).to(dev)
        IV = ma.InverseRealVectorSHT(nlat, nlon, lmax=L, mmax=M, grid=grid).to(dev)
        S = ma.RealSHT(nlat, nlon, lmax=L, mmax=M, grid=grid).to(dev)
        I = ma.InverseRealSHT(nlat, nlon, lmax=L, mmax=M, grid=grid).to(dev)
        Rp = ops.round32(P)
        F = torch.randn(M, nlat, 2, 2 * Rp, device=dev)
        Sc = torch.randn(L, M, 2, 2 * Rp, device=dev)
        for name, vec, sca in (("analysis ", lambda: ops.vector_legendre(F, V._mats(), 0), lambda: ops.legendre_analysis(F, S.weights_t, L)),
                               ("synthesis", lambda: ops.vector_legendre(Sc, IV._mats(), 1), lambda: ops.legendre_synthesis(Sc, I.pct, nlat))):
            ts = timeit(sca, reps=20, warm=3)
            tv = timeit(vec, reps=20, warm=3)
            ts2 = timeit(sca, reps=20, warm=3)                  # the scalar launch again: drift of the box within the run
            print(f"vsht {name} {nlat}x{nlon} L=M={L} P={P}: vector {tv:7.3f} ms  scalar(2P planes) {ts:7.3f} / {ts2:7.3f} ms  ratio {tv / min(ts, ts2):5.2f}")
        tz = timeit(lambda: ops.vector_legendre(Sc[..., :Rp].contiguous(), IV._mats(), 3), reps=20, warm=3)
        print(f"vsht synthesis t=0 {nlat}x{nlon} P={P}: {tz:7.3f} ms (includes one S copy)")
        del V, IV, S, I, F, Sc


def escore():
    """energy-score stages 1 (mk_escore_sums) and 3 (mk_escore_grad) at 721 x 1440, C = 73, B = 1 as a fraction of HBM peak on
    ALGORITHMIC traffic — (E + 1) plane reads forward, (E + 1) reads + E writes backward — beside crps_kernel at the same shape
    and, for E = 2 only (its pair tensor grows with E^2), a torch restatement of the reference formula"""
    from makani_amd import _lib
    from makani_amd._lib import lib, ptr, stream, check
    PEAK = 8.0e12
    H, W, C, B = 721, 1440, 73, 1
    N = H * W
    q = torch.rand(N, device=dev) / N
    for E in (2, 8, 16):
        for dt in (torch.float32, torch.bfloat16):
            f = torch.randn(B, E, C, N, device=dev).to(dt)
            o = torch.randn(B, C, N, device=dev)
            kind = _lib.dtype_code(f)
            K = E + E * (E - 1) // 2
            sums = torch.empty(B, C, 1, K, device=dev)
            ws = torch.empty(lib().mk_escore_sums_workspace(B, E, C, N, 1, 0), device=dev)
            loss, table = torch.empty(B, 1, device=dev), torch.empty(B, 1, 1, K, device=dev)
            gout, gf = torch.ones(B, 1, device=dev), torch.empty_like(f)

            def fwd():
                check(lib().mk_escore_sums(ptr(f), kind, ptr(o), ptr(q), None, ptr(sums), ptr(ws), B, E, C, N, 1, 0, 2.0, stream()))

            def bwd():
                check(lib().mk_escore_grad(ptr(f), kind, ptr(o), ptr(q), None, ptr(table), ptr(gout), ptr(gf), B, E, C, 1, N, 1, 0, 2.0, stream()))

            fwd()
            check(lib().mk_escore_finish(ptr(sums), None, 0, ptr(loss), ptr(table), B, E, C, 1, 1, 2.0, 1.0, 1.0, 1e-6, stream()))
            es = f.element_size()
            bytes_f = C * N * (E * es + 4)
            bytes_b = C * N * (E * es + 4 + E * es)
            tf, tb = timeit(fwd, reps=10, warm=2), timeit(bwd, reps=10, warm=2)
            crps = ma.CRPSLoss(img_shape=(H, W), crop_shape=(H, W), crop_offset=(0, 0), channel_names=[str(c) for c in range(C)],
                               grid_type="equiangular").to(dev)
            f5, o4 = f.view(B, E, C, H, W), o.view(B, C, H, W)
            tc = timeit(lambda: crps(f5, o4), reps=10, warm=2)
            pct = lambda nbytes, ms: nbytes / (ms * 1e-3) / PEAK * 100
            line = (f"escore E={E:2d} {str(dt)[6:]:9s} sums {tf:7.3f} ms {pct(bytes_f, tf):5.1f} % of peak | "
                    f"grad {tb:7.3f} ms {pct(bytes_b, tb):5.1f} % | crps fwd {tc:7.3f} ms {pct(bytes_f, tc):5.1f} %")
            if E == 2 and dt == torch.float32:
                def torch_ref():
                    fe = torch.moveaxis(f, 1, 0)
                    d = ((fe[0] - fe[1]).abs().pow(2.0) * q).sum(-1).sum(-1, keepdim=True)
                    s = ((o.unsqueeze(0) - fe).abs().pow(2.0) * q).sum(-1).sum(-1, keepdim=True)
                    return s.sqrt().sum(0) / E - 0.5 * d.sqrt() * 2.0 * E / (E * E * (E - 1))
                line += f" | torch formula fwd {timeit(torch_ref, reps=5, warm=1):7.3f} ms"
            print(line, flush=True)
            del f, o, gf


def losses():
    """SpectralAMSELoss, EnsembleNLLLoss and GaussianMMDLoss, forward + backward, at 721 x 1440, C = 73, B = 1, E = 2 and 16,
    beside the reference formula in plain torch on the same GPU, in the same process, the two timed in turn over three rounds.
    Achieved bytes/s over the ALGORITHMIC traffic as a fraction of the HBM roof: NLL reads the members once (plus observation
    and quadrature weights) and writes their gradient once; AMSE (kernels alone, on coefficient planes) reads two planes and
    writes two.  MMD's torch formula is timed at E = 2 only (its pair tensor grows with E^2)."""
    PEAK = 8.0e12
    H, W, C, B = 721, 1440, 73, 1
    N = H * W
    kw = dict(img_shape=(H, W), crop_shape=(H, W), crop_offset=(0, 0), channel_names=[str(c) for c in range(C)], grid_type="equiangular")
    pct = lambda nbytes, ms: nbytes / (ms * 1e-3) / PEAK * 100

    def fb(fn, *xs):
        def run():
            for x in xs:
                x.grad = None
            fn().sum().backward()
        return run

    # ---- AMSE: the two kernels on coefficient planes, and the module with its transforms
    amse = ma.SpectralAMSELoss(**kw).to(dev)
    L, M = amse.sht.lmax, amse.sht.mmax
    X = torch.randn(B, C, L, M, dtype=torch.complex64, device=dev).requires_grad_(True)
    Y = torch.randn(B, C, L, M, dtype=torch.complex64, device=dev).requires_grad_(True)
    from makani_amd.losses import AmseSumsFn

    def finish(sums):
        a, b, c = sums.unbind(-1)
        coh = c / torch.sqrt(a * b + 1e-6)
        return (torch.square(torch.sqrt(a) - torch.sqrt(b)) + 2 * torch.maximum(a, b) * (1 - coh)).sum(-1)

    def amse_torch():
        inv = 1.0 / (4.0 * math.pi)
        xx, yy, xy = torch.square(torch.abs(X)), torch.square(torch.abs(Y)), torch.real(X * Y.conj())
        return finish(torch.stack([inv * (v[..., 0] + 2 * torch.sum(v[..., 1:], dim=-1)) for v in (xx, yy, xy)], dim=-1))

    k_amse = fb(lambda: finish(AmseSumsFn.apply(X, Y, None, 0, 0)), X, Y)
    t_amse = fb(amse_torch, X, Y)
    nbytes = 4 * B * C * L * M * 8 + 2 * B * C * L * M * 8         # backward: two planes read, two written; forward: two read
    for rnd in range(3):
        tk, tt = timeit(k_amse, reps=30, warm=3), timeit(t_amse, reps=10, warm=2)
        print(f"losses AMSE kernels on ({B * C}, {L}, {M}) planes round {rnd}: fwd + bwd {tk:7.3f} ms {pct(nbytes, tk):5.1f} % of the HBM roof "
              f"({nbytes / 1e9:.2f} GB) | torch formula {tt:7.3f} ms = {tt / tk:5.1f} x", flush=True)
    prd = torch.randn(B, C, H, W, device=dev).requires_grad_(True)
    tar = torch.randn(B, C, H, W, device=dev)
    tm = timeit(fb(lambda: amse(prd, tar), prd), reps=10, warm=2)
    print(f"losses AMSE module (two analyses, kernels, one adjoint analysis) fwd + bwd {tm:7.3f} ms", flush=True)
    del X, Y, prd, tar

    q = (torch.rand(N, device=dev) / N).view(1, 1, N)
    for E in (2, 16):
        f = torch.randn(B, E, C, H, W, device=dev).requires_grad_(True)
        o = torch.randn(B, C, H, W, device=dev)
        # ---- NLL
        nll = ma.EnsembleNLLLoss(**kw).to(dev)

        def nll_torch():
            s2, mu = torch.var_mean(f.reshape(B, E, C, N), dim=1, correction=0)
            s2 = torch.clamp(s2, min=1e-12)
            return torch.sum(0.5 * (torch.log(s2) + torch.square(o.reshape(B, C, N) - mu) / s2) * q, dim=-1)

        nbytes = C * N * 4 * (2 * (E + 1) + E) + 2 * N * 4          # forward and backward read members + observation, backward writes E
        k, t = fb(lambda: nll(f, o), f), fb(nll_torch, f)
        for rnd in range(3):
            tk, tt = timeit(k, reps=20, warm=3), timeit(t, reps=5, warm=2)
            print(f"losses NLL E={E:2d} round {rnd}: fwd + bwd {tk:7.3f} ms {pct(nbytes, tk):5.1f} % of the HBM roof ({nbytes / 1e9:.2f} GB) | "
                  f"torch formula {tt:7.3f} ms = {tt / tk:5.1f} x", flush=True)
        # ---- MMD
        mmd = ma.GaussianMMDLoss(sigma=4.0, **kw).to(dev)

        def mmd_torch():
            fe = torch.moveaxis(f, 1, 0).reshape(E, B, C, N)
            sp = torch.sum((fe.unsqueeze(1) - fe.unsqueeze(0)).abs().pow(2.0) * q, dim=-1)
            sk = torch.sum((o.reshape(1, B, C, N) - fe).abs().pow(2.0) * q, dim=-1)
            sp, sk = torch.exp(-0.5 * torch.square(sp) / 4.0), torch.exp(-0.5 * torch.square(sk) / 4.0)
            sp = torch.where(torch.eye(E, device=dev).bool().reshape(E, E, 1, 1), 0.0, sp)
            return sk.sum(0) / E - 0.5 * sp.sum(dim=(0, 1)) * E / (E * E * (E - 1))

        k = fb(lambda: mmd(f, o), f)
        for rnd in range(3):
            tk = timeit(k, reps=10, warm=2)
            line = f"losses MMD E={E:2d} round {rnd}: fwd + bwd {tk:7.3f} ms {pct(nbytes, tk):5.1f} % of the HBM roof on single-pass traffic"
            if E == 2:
                tt = timeit(fb(mmd_torch, f), reps=5, warm=2)
                line += f" | torch formula {tt:7.3f} ms = {tt / tk:5.1f} x"
            print(line, flush=True)
        del f, o
    coherence()


def coherence():
    """The per-degree ensemble Gram kernels (csrc/egram.hip) with the finish of SpectralCoherenceLoss, forward + backward, on the
    coefficient planes of a 721 x 1440 grid (L = M = 360), C = 73, B = 1, E = 2 and 16, beside the reference formulation in plain
    torch (broadcast products, the (E, E, B, C, L, M) tensor) on the same GPU, in the same process, the two timed in turn over
    three rounds.  Achieved bytes/s over the SINGLE-PASS traffic (members + observation read in each direction, the member
    gradient written) as a fraction of the HBM roof; the kernel re-reads tiles for E > 7 and skips the orders m > l.  Also part
    of `losses`."""
    from makani_amd.losses import EGRAM_FULL, EnsembleGramFn, _pair_decoherence, egram_weights
    PEAK = 8.0e12
    B, C, L = 1, 73, 360
    M = L
    q, tri_off = egram_weights(L, M)
    q = q.to(dev)
    qt = q * (4.0 * math.pi)
    eps = 1.0e-6
    pct = lambda nbytes, ms: nbytes / (ms * 1e-3) / PEAK * 100
    for E in (2, 16):
        f = torch.randn(B, E, C, L, M, dtype=torch.complex64, device=dev).requires_grad_(True)
        o = torch.randn(B, C, L, M, dtype=torch.complex64, device=dev)
        n = E + 1

        def finish(psd_f, psd_o, cross, spread):
            coh = (1.0 - cross / torch.sqrt(psd_f * psd_o + eps)).sum(dim=-1) / E - 0.5 * spread
            return ((psd_f - psd_o).square().sum(dim=-1) / E + 2.0 * psd_o.squeeze(-1) * coh).sum(dim=-1)

        def kernel():
            f.grad = None
            G = EnsembleGramFn.apply(f, o, q, EGRAM_FULL, tri_off, [])
            psd_f = G[..., :E]
            finish(psd_f, G[..., E:n], G[..., n:n + E], _pair_decoherence(psd_f, G[..., n + E:], E, eps)).sum().backward()

        def formula():
            f.grad = None
            fe = torch.moveaxis(f, 1, 0) / math.sqrt(4.0 * math.pi)
            oe = o.unsqueeze(0) / math.sqrt(4.0 * math.pi)
            psd_f = (qt * fe.abs().square()).sum(dim=-1)
            psd_o = (qt * oe.abs().square()).sum(dim=-1)
            pairs = (qt * (fe.unsqueeze(0).conj() * fe.unsqueeze(1)).real).sum(dim=-1)
            cross = (qt * (fe.conj() * oe).real).sum(dim=-1)
            coh_f = pairs / torch.sqrt(psd_f.unsqueeze(0) * psd_f.unsqueeze(1) + eps)
            spread = torch.where(torch.eye(E, device=dev).bool().reshape(E, E, 1, 1, 1), 0.0, 1.0 - coh_f).sum(dim=(0, 1)) / (E * (E - 1))
            finish(torch.movedim(psd_f, 0, -1), torch.movedim(psd_o, 0, -1), torch.movedim(cross, 0, -1), spread).sum().backward()

        nbytes = B * C * L * M * 8 * (2 * n + E)
        for rnd in range(3):
            tk, tt = timeit(kernel, reps=20, warm=3), timeit(formula, reps=3, warm=1)
            print(f"coherence E={E:2d} on ({B}, {E}, {C}, {L}, {M}) round {rnd}: fwd + bwd {tk:7.3f} ms {pct(nbytes, tk):5.1f} % of the HBM roof "
                  f"on single-pass traffic ({nbytes / 1e9:.2f} GB) | torch formulation {tt:7.3f} ms = {tt / tk:5.1f} x", flush=True)
        del f, o


def metrics():
    """The plane sums of the validation metrics (csrc/metrics.hip), forward only, at 721 x 1440, C = 73, B = 1, E = 2 and 16, beside
    the reference formulation in plain torch on the same GPU, in the same process, the two timed in turn over three rounds.
    Achieved bytes/s over the ALGORITHMIC traffic: x + y (+ bias, weight) once for the deterministic sums, E + 1 planes once for
    the ensemble sums (plus the quadrature weights)."""
    from makani_amd import metrics as mm
    PEAK = 8.0e12
    H, W, C, B = 721, 1440, 73, 1
    N = H * W
    quad = ma.GridQuadrature("naive", (H, W)).to(dev)
    q = quad.quad_weight
    rate = lambda nbytes, ms: f"{nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s = {nbytes / (ms * 1e-3) / PEAK * 100:5.1f} % of the HBM roof"
    with torch.no_grad():
        x, y = torch.randn(B, C, H, W, device=dev), torch.randn(B, C, H, W, device=dev)
        bias, w = torch.randn(C, H, W, device=dev), torch.rand(B, C, H, W, device=dev) + 0.5

        def rmse_torch():
            return torch.sum(torch.square(x - y) * q, dim=(-2, -1))

        def acc_torch():
            xb, yb = x - bias, y - bias
            return (torch.sum(xb * yb * q, dim=(-2, -1)), torch.sum(torch.square(xb) * q, dim=(-2, -1)), torch.sum(torch.square(yb) * q, dim=(-2, -1)))

        forms = [("RMSE sum", lambda: ma.deterministic_sums(x, y, quad, which=mm.SUM_L2), rmse_torch, (2 * B * C + 1) * N * 4),
                 ("ACC sums, bias", lambda: ma.deterministic_sums(x, y, quad, bias=bias, which=mm.SUM_ACC), acc_torch, (2 * B * C + C + 1) * N * 4),
                 ("all five, bias, weight", lambda: ma.deterministic_sums(x, y, quad, bias=bias, weight=w),
                  lambda: (rmse_torch(), acc_torch(), torch.sum(torch.abs(x - y) * q, dim=(-2, -1))), (3 * B * C + C + 1) * N * 4)]
        for name, k, t, nbytes in forms:
            for rnd in range(3):
                tk, tt = timeit(k, reps=30, warm=3), timeit(t, reps=10, warm=2)
                print(f"metrics {name} round {rnd}: {tk:7.3f} ms {rate(nbytes, tk)} ({nbytes / 1e9:.2f} GB) | torch formulation"
                      f"{' (RMSE + ACC + L1, no weight)' if name.startswith('all') else ''} {tt:7.3f} ms = {tt / tk:5.1f} x", flush=True)
        del x, y, bias, w
        for E in (2, 16):
            f, o = torch.randn(B, E, C, H, W, device=dev), torch.randn(B, C, H, W, device=dev)
            f4, o3, qn = f.reshape(B, E, C, N), o.reshape(B, C, N), q.reshape(-1)
            nbytes = ((E + 1) * B * C + 1) * N * 4

            def ssr_torch():
                mean = torch.sum(f, dim=1) / float(E)
                skill = torch.square(mean - o)
                spread = torch.sum(torch.square(mean.unsqueeze(1) - f), dim=1) / float(E - 1)
                return torch.sum(skill * q, dim=(-2, -1)), torch.sum(spread * q, dim=(-2, -1))

            def hist_torch():
                fs, _ = torch.sort(torch.moveaxis(f4, 1, -1), dim=-1, descending=False, stable=True)
                ins = torch.searchsorted(fs.contiguous(), o3.unsqueeze(-1).contiguous(), side="right").squeeze(-1)
                return torch.sum(torch.nn.functional.one_hot(ins, num_classes=E + 1).to(torch.float32) * qn.reshape(1, 1, -1, 1), dim=2)

            forms = [("skill + spread", lambda: mm._ens_launch(f4, o3, qn, None, 3), ssr_torch),
                     ("rank histogram", lambda: mm._ens_launch(f4, o3, qn, None, 4), hist_torch),
                     ("all three", lambda: mm._ens_launch(f4, o3, qn, None, 7), lambda: (ssr_torch(), hist_torch()))]
            for name, k, t in forms:
                for rnd in range(3):
                    tk, tt = timeit(k, reps=20, warm=3), timeit(t, reps=3, warm=1)
                    print(f"metrics E={E:2d} {name} round {rnd}: {tk:7.3f} ms {rate(nbytes, tk)} ({nbytes / 1e9:.2f} GB) | torch formulation "
                          f"{tt:8.3f} ms = {tt / tk:6.1f} x", flush=True)
            del f, o, f4, o3


def noise():
    """the diffusion noise's autoregressive update (mk_noise_update + mk_noise_advance) at the FourCastNet3 recipe's size, beside
    the reference's torch formulation of the same update on GPU tensors and a plain device copy of the state as the bandwidth
    yardstick; traffic counted as one read and one write of the state.  Three rounds, the three timed in turn within each; then
    the inverse SHT's share of update + forward."""
    T, C, nlat, nlon = 1, 8, 721, 1440
    for B in (16, 2):
        m = ma.DiffusionNoiseS2((nlat, nlon), B, C, num_time_steps=T, kT=[0.5 * (100.0 * 2 ** c / 6370.0) ** 2 for c in range(C)]).to(dev)
        m.update(replace_state=True)
        st = m.state
        nbytes = 2 * st.numel() * 4
        twin, dst = st.clone(), torch.empty_like(st)
        gen = torch.Generator(device=dev).manual_seed(333)

        def torch_update():                                   # normal_, scale, damp + add, copy_: the reference's operations
            xi = torch.empty_like(twin).normal_(mean=0.0, std=1.0, generator=gen)
            eta = m.sigma_l * xi
            twin.copy_(m.phi * twin + eta)

        for rnd in range(3):
            tk = timeit(m.update, reps=50, warm=3)
            tt = timeit(torch_update, reps=20, warm=2)
            tc = timeit(lambda: dst.copy_(st), reps=50, warm=3)
            print(f"noise AR update B={B:2d} C={C} {nlat}x{nlat} ({nbytes / 2e9:.2f} GB state) round {rnd}: kernel {tk:7.3f} ms "
                  f"{nbytes / tk / 1e9:6.2f} TB/s = {tc / tk * 100:5.1f} % of the copy rate | copy {tc:7.3f} ms {nbytes / tc / 1e9:6.2f} TB/s | "
                  f"torch formulation {tt:7.3f} ms = {tt / tk:5.1f} x the kernel", flush=True)
        with torch.no_grad():
            tf = timeit(lambda: m(), reps=5, warm=2)
            tr = timeit(lambda: m.update(replace_state=True), reps=20, warm=2)
        print(f"noise B={B:2d}: replace {tr:7.3f} ms | forward (inverse SHT of {B * T * C} planes) {tf:7.3f} ms = "
              f"{tf / (tk + tf) * 100:5.1f} % of update + forward", flush=True)
        del m, st, twin, dst


def noise_shard():
    """mk_noise_update_shard at the boxes one rank of BASELINE configs[3] / [4] owns (721 x 1440, lmax = mmax = 721, 8 channels,
    B = 2, T = 1, the autoregressive rule; l split [361, 360] under h = 2 and [181, 180, 180, 180] under h = 4, m split
    [361, 360]) beside mk_noise_update on a whole array of the same number of elements; traffic counted as one read and one write
    of the state.  Seven rounds, the two timed in turn within each; min / median / max over the rounds."""
    from makani_amd import _lib
    L_ = _lib.lib()
    B, T, C, lmax, mmax = 2, 1, 8, 721, 721
    rng = torch.tensor([333, 0], dtype=torch.int64, device=dev)
    phi = torch.full((C,), 0.8, device=dev)
    for name, (r0, Rl), (m0, ml) in (("h2 w2 rank (0, 0)", (0, 361), (0, 361)), ("h2 w2 rank (0, 1)", (0, 361), (361, 360)),
                                     ("h2 w2 rank (1, 0)", (361, 360), (0, 361)), ("h2 w2 rank (1, 1)", (361, 360), (361, 360)),
                                     ("h4 w2 rank (0, 0)", (0, 181), (0, 361)), ("h4 w2 rank (0, 1)", (0, 181), (361, 360)),
                                     ("h4 w2 rank (3, 0)", (541, 180), (0, 361)), ("h4 w2 rank (3, 1)", (541, 180), (361, 360))):
        box, whole = torch.randn(B, T, C, Rl, ml, 2, device=dev), torch.randn(B, T, C, Rl, ml, 2, device=dev)
        sigma = torch.rand(C, Rl, device=dev) * 0.1
        nbytes = 2 * box.numel() * 4
        head = (_lib.ptr(sigma), _lib.ptr(phi), _lib.ptr(rng), 1, B, T, C)

        def shard():
            _lib.check(L_.mk_noise_update_shard(_lib.ptr(box), None, *head, lmax, 2 * mmax, r0, Rl, 2 * m0, 2 * ml, 0, _lib.stream()))

        def serial():
            _lib.check(L_.mk_noise_update(_lib.ptr(whole), None, *head, Rl, ml, 0, _lib.stream()))

        ts, tw = [], []
        for _ in range(7):
            ts.append(timeit(shard, reps=200, warm=5))
            tw.append(timeit(serial, reps=200, warm=5))
        ts.sort()
        tw.sort()
        print(f"noise shard {name}: rows [{r0}, {r0 + Rl}) x orders [{m0}, {m0 + ml}) ({nbytes / 2e6:.1f} MB state) | shard "
              f"{ts[0] * 1e3:6.1f} / {ts[3] * 1e3:6.1f} / {ts[6] * 1e3:6.1f} us = {nbytes / ts[3] / 1e6:7.1f} GB/s | whole array of the "
              f"same size {tw[0] * 1e3:6.1f} / {tw[3] * 1e3:6.1f} / {tw[6] * 1e3:6.1f} us = {nbytes / tw[3] / 1e6:7.1f} GB/s | "
              f"shard / whole {ts[3] / tw[3]:5.2f}", flush=True)
        del box, whole


def preproc():
    """Preprocessor2D's fused stages (csrc/preproc.hip) at 721 x 1440, B = 1, C = 73, U = 1, S = 3, fp32, forward only, modes "none"
    and "mean", n_history 0 and 1, beside the torch composition of the reference's operations (cat, weighted quadrature sums, tile,
    sub, div, cat; sub, mul, add) on the same tensors, the two timed in turn over three rounds, every timing over a window of at
    least 0.5 s.  Algorithmic bytes: statistics one read of the sources; assemble one read of sources and static planes plus one
    write of the network input; finish one read of yn and the bias field plus one write."""
    PEAK = 8.0e12
    H, W, B, C, U, S = 721, 1440, 1, 73, 1, 3
    N = H * W
    rate = lambda nbytes, ms: f"{nbytes / (ms * 1e-3) / PEAK * 100:5.1f} % of the HBM roof"

    def timed(fn):
        once = max(timeit(fn, reps=3, warm=2), 1e-3)
        return timeit(fn, reps=max(5, int(math.ceil(500.0 / once))), warm=1)

    for mode in ("none", "mean"):
        for nh in (0, 1):
            T, J = nh + 1, C + U
            with torch.no_grad():
                win = torch.randn(B, T * C, H, W, device=dev) * 2 + 1
                xz = torch.randn(B, T, U, H, W, device=dev)
                static, bias = torch.randn(1, S, H, W, device=dev), torch.randn(1, C, H, W, device=dev)
                yn = torch.randn(B, C, H, W, device=dev)
                pre = ma.Preprocessor2D(img_shape=(H, W), n_history=nh, history_normalization_mode=mode, static_features=static,
                                        bias_correction=bias).to(dev)
                pre.train()
                pre.cache_unpredicted_features(None, None, xz, None)
                q = ma.GridQuadrature("naive", (H, W), normalize=True).to(dev).quad_weight
                wts = torch.full((1, T, 1, 1, 1), 1.0 / T, device=dev)
                stats = {}

                def torch_assemble():
                    xo = torch.cat([win.reshape(B, T, C, H, W), xz], dim=2)
                    xf = xo.flatten(1, 2)
                    if mode != "none":
                        mean = torch.sum(torch.sum(xo * wts * q, dim=(-2, -1)), dim=1, keepdim=True).reshape(B, 1, J, 1, 1)
                        std = torch.sqrt(torch.sum(torch.sum(torch.square(xo - mean) * wts * q, dim=(-2, -1)), dim=1, keepdim=True))
                        stats["mean"], stats["std"] = mean.reshape(B, J, 1, 1), std.reshape(B, J, 1, 1)
                        xf = (xf - torch.tile(stats["mean"], (1, T, 1, 1))) / torch.tile(stats["std"], (1, T, 1, 1))
                    return torch.cat([xf, torch.tile(static, (B, 1, 1, 1))], dim=1)

                def torch_finish():
                    y = yn - bias
                    return y * stats["std"][:, :C] + stats["mean"][:, :C] if mode != "none" else y

                b_stats = (B * T * J + 1) * N * 4 if mode != "none" else 0
                b_asm = (B * T * J + S + B * (T * J + S)) * N * 4
                b_fin = (2 * B * C + C) * N * 4
                err = (pre.assemble(win) - torch_assemble()).abs().max().item(), (pre.finish(yn) - torch_finish()).abs().max().item()
                for rnd in range(3):
                    ta, tta = timed(lambda: pre.assemble(win)), timed(torch_assemble)
                    tf, ttf = timed(lambda: pre.finish(yn)), timed(torch_finish)
                    print(f"preproc {mode:4s} n_history={nh} round {rnd}: assemble {ta:7.3f} ms {rate(b_stats + b_asm, ta)} "
                          f"({(b_stats + b_asm) / 1e9:.2f} GB) | torch composition {tta:7.3f} ms = {tta / ta:5.2f} x | finish {tf:7.3f} ms "
                          f"{rate(b_fin, tf)} ({b_fin / 1e9:.2f} GB) | torch composition {ttf:7.3f} ms = {ttf / tf:5.2f} x | "
                          f"max |fused - torch| {err[0]:.1e} {err[1]:.1e}", flush=True)
                if mode != "none":
                    from makani_amd import preprocessor as pp
                    src = pp._Src(win, xz, None, T)
                    ts = timed(lambda: pp._stats(src, q, pre.history_time_weights))
                    tasm = timed(lambda: pp._assemble(src, static[0], pre.history_mean.reshape(B, J), pre.history_std.reshape(B, J)))
                    print(f"preproc {mode:4s} n_history={nh}: statistics {ts:7.3f} ms {rate(b_stats, ts)} ({b_stats / 1e9:.2f} GB) | assemble "
                          f"launch {tasm:7.3f} ms {rate(b_asm, tasm)} ({b_asm / 1e9:.2f} GB)", flush=True)
                del win, xz, static, bias, yn, pre


def constraints():
    """The output constraints (csrc/constraints.hip) at 721 x 1440, B = 1, C = 73 (8 surface channels, u v z t q on 13 levels),
    forward + backward, f32 and bf16: the hydrostatic wrapper (61 -> 73 channels) and the projection, dry and moist, and the
    "softplus" non-negativity clamp of the 13 q channels and tcwv; beside the reference's formulation in plain torch (gather,
    .float(), scale and bias, a dense F.conv2d, divide, re-normalise, cast, index_copy; backward by autograd) on the same tensors
    in the same process, the two timed in turn over three rounds, every timing over a window of at least 0.5 s.  Algorithmic
    bytes: one read of the input and one write of the output per direction."""
    import torch.nn.functional as F
    from makani_amd import constraints as mc
    PEAK = 8.0e12
    H, W, B = 721, 1440, 1
    N = H * W
    levels = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
    names = ["u10m", "v10m", "u100m", "v100m", "t2m", "sp", "msl", "tcwv"] + [f"{v}{p}" for v in "uvztq" for p in levels]
    C = len(names)
    gen = torch.Generator().manual_seed(1)
    bias, scale = torch.zeros(1, C, 1, 1), torch.ones(1, C, 1, 1)
    for i, n in enumerate(names):
        if n[1:].isdigit():
            k = math.log(1000.0 / int(n[1:])) / math.log(20.0)
            b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3), "t": (285.0 - 70.0 * k, 15.0), "q": (2.0e-3, 2.0e-3), "u": (5.0, 10.0), "v": (0.0, 8.0)}[n[0]]
            bias[0, i], scale[0, i] = b, s
    EPS = mc.Q_CORRECTION_MOIST_AIR

    def timed(fn):
        once = max(timeit(fn, reps=3, warm=2), 1e-3)
        return timeit(fn, reps=max(5, int(math.ceil(500.0 / once))), warm=1)

    def torch_wrapper(m):
        L, moist = m.num_levels, m.use_moist_air_formula
        def f(x):
            u = x.to(torch.float32) * m.inp_scale + m.inp_bias
            if moist:
                us = u.clone()
                us[:, 0] = u[:, 0] * (1.0 + EPS * u[:, L + 1])
                u = us
            v = F.conv2d(u, m.mapping.unsqueeze(-1).unsqueeze(-1))
            if moist:
                v[:, m.t_idx] = v[:, m.t_idx] / (1.0 + EPS * v[:, m.q_idx])
            return ((v - m.out_bias) / m.out_scale).to(x.dtype)
        return f

    def torch_projection(m):
        L, moist = m.num_levels, m.use_moist_air_formula
        def f(x):
            xp = x[:, m.channel_indices].float() * m.scale_sub + m.bias_sub
            if moist:
                q = x[:, m.q_indices].float() * m.q_scale + m.q_bias
                mult = torch.cat([1.0 + EPS * q, torch.ones_like(xp[:, L:])], dim=1)
                xp = xp * mult
            xp = xp - m.strength * (F.conv2d(xp, m.proj.unsqueeze(-1).unsqueeze(-1)) - m.off)
            if moist:
                xp = xp / mult
            return x.index_copy(1, m.channel_indices, ((xp - m.bias_sub) / m.scale_sub).to(x.dtype))
        return f

    def torch_nonneg(m):
        def f(x):
            off = m.offset.to(x.dtype)
            ws = x[:, m.channel_indices] + off
            w = m.leak * ws + (1.0 - m.leak) * m.eps * (F.softplus(ws / m.eps) - math.log(2.0)) - off
            return x.index_copy(1, m.channel_indices, w.to(x.dtype))
        return f

    layers = []
    for moist in (False, True):
        layers.append((f"wrapper {'moist' if moist else 'dry  '}", mc._HydrostaticBalanceWrapper(names, bias, scale, p_min=50, p_max=1000,
                                                                                                use_moist_air_formula=moist), torch_wrapper))
    for moist in (False, True):
        layers.append((f"projection {'moist' if moist else 'dry  '}", mc.HydrostaticBalanceProjection(names, bias, scale, p_min=50, p_max=1000,
                                                                                                   use_moist_air_formula=moist), torch_projection))
    layers.append(("nonneg softplus", mc.NonNegativeConstraint(names, [f"q{p}" for p in levels] + ["tcwv"], bias, scale, mode="softplus"),
                   torch_nonneg))
    for label, mod, make in layers:
        mod = mod.to(dev).train()
        cin = mod.mapping.shape[1] if hasattr(mod, "mapping") else C
        tfn = make(mod)
        for dt in (torch.float32, torch.bfloat16):
            x = torch.randn(B, cin, H, W, generator=gen).to(dt).to(dev).requires_grad_(True)
            g = torch.randn(B, C, H, W, generator=gen).to(dt).to(dev)
            nbytes = 2 * (cin + C) * B * N * x.element_size()

            def ours():
                return torch.autograd.grad(mod(x), x, g)[0]

            def composed():
                return torch.autograd.grad(tfn(x), x, g)[0]

            err = ((mod(x).detach().float() - tfn(x).detach().float()).abs().max().item(),
                   (ours().float() - composed().float()).abs().max().item())
            for rnd in range(3):
                t, tt = timed(ours), timed(composed)
                print(f"constraints {label:16s} {str(dt)[6:]:8s} round {rnd}: forward + backward {t:7.3f} ms = {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s "
                      f"= {nbytes / (t * 1e-3) / PEAK * 100:5.1f} % of the HBM roof ({nbytes / 1e9:.2f} GB) | torch formulation {tt:7.3f} ms = "
                      f"{tt / t:5.2f} x | max |kernel - torch| {err[0]:.1e} {err[1]:.1e}", flush=True)
            del x, g


def interpolant():
    """The stochastic-interpolant stepper (csrc/interpolant.hip) at 721 x 1440, C = 73, B = 1, U = 1, St = 3, fp32: the training
    assemble for S' = 4 time samples (one launch) and one Foellmer sampler step (one launch), each beside the reference's op
    sequence in plain torch on the same tensors in the same process (expand_time's repeats, the two three-term broadcasts, tile and
    cat; for the step bhat, the score correction, the noise term and the cat of the next input), the two timed in turn over three
    rounds, every timing over a window of at least 0.5 s.  Algorithmic bytes: every source read once, every output written once.
    The torch sequence's compute ops are counted by a dispatch mode (views left out): each is at least one launch."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from makani_amd.interpolant import step_coefficients
    PEAK = 8.0e12
    H, W, B, C, U, St, Sp, eps = 721, 1440, 1, 73, 1, 3, 4, 0.7
    N, Cin = H * W, 2 * C + U + St + 1
    gen = torch.Generator().manual_seed(1)
    x0, x1, z, bnet = (torch.randn(B, C, H, W, generator=gen).to(dev) for _ in range(4))
    xu, static = torch.randn(B, U, H, W, generator=gen).to(dev), torch.randn(1, St, H, W, generator=gen).to(dev)
    s = torch.rand(B, Sp, generator=gen).to(dev)
    VIEWS = ("view", "reshape", "expand", "unsqueeze", "squeeze", "slice", "select", "alias", "detach", "transpose", "permute", "as_strided", "t.")

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not any(v in str(func) for v in VIEWS):
                Count.n += 1
            return func(*args, **(kwargs or {}))

    def counted(fn):
        Count.n = 0
        with Count():
            fn()
        return Count.n

    def timed(fn):
        once = max(timeit(fn, reps=3, warm=2), 1e-3)
        return timeit(fn, reps=max(5, int(math.ceil(500.0 / once))), warm=1)

    def expand_time(x, n):
        return x.unsqueeze(1).repeat(1, n, *[1] * (x.dim() - 1))

    sig = lambda t: eps * (1.0 - t)

    def torch_train():
        inpu = expand_time(xu, Sp).flatten(0, 1)
        stat = expand_time(torch.tile(static, (B, 1, 1, 1)), Sp).flatten(0, 1)
        a, t = expand_time(x0, Sp), expand_time(x1, Sp)
        noise = z.unsqueeze(1)
        sr = s.reshape(B, Sp, 1, 1, 1)
        inter = (1.0 - sr) * a + torch.square(sr) * t + (torch.sqrt(sr) * sig(sr)) * noise
        drift = -1.0 * a + (2.0 * sr) * t + (torch.sqrt(sr) * (-1.0 * eps)) * noise
        sp = torch.tile(s.flatten().reshape(-1, 1, 1, 1), (1, 1, H, W))
        return torch.cat([a.flatten(0, 1), inter.flatten(0, 1), inpu, stat, sp], dim=-3), drift.flatten(0, 1)

    def ours_train():
        return ops.si_assemble(x0, x1, z, s, xu, static[0], eps)

    si, ds = 0.5, 0.25
    sv = torch.full((B, 1, 1, 1), si, device=dev)
    dsv = torch.tensor(ds, device=dev)
    coef = step_coefficients(si, ds, eps, foellmer=True)
    x_prev = ours_train()[0][:B].contiguous()

    def torch_step():
        x, b = x_prev[:, C:2 * C], bnet
        sg = sig(sv)
        gsq = torch.abs(2.0 * torch.square(sg) * torch.where(sv > 0, sv * (2.0 * sv) / torch.square(sv), 2.0) - 2.0 * sv * sg * (-1.0 * eps)
                        - torch.square(sg))
        As = 1.0 / (sv * sg * ((2.0 * sv) * sg - torch.square(sv) * (-1.0 * eps)))
        cs = x * (2.0 * sv) + (torch.square(sv) * -1.0 - (2.0 * sv) * (1.0 - sv)) * x0
        bhat = b + 0.5 * (gsq - torch.square(sg)) * (As * (torch.square(sv) * b - cs))
        xn = x + bhat * dsv
        xn = xn + torch.sqrt(gsq * dsv) * z
        sp = torch.tile(torch.full((B,), si + ds, device=dev).reshape(-1, 1, 1, 1), (1, 1, H, W))
        return torch.cat([x0, xn, xu, static.expand(B, -1, -1, -1), sp], dim=-3)

    def ours_step():
        return ops.si_step(x_prev[:, C:2 * C], bnet, x0, z, xu, static[0], coef, si + ds)

    b_train = 4 * N * (B * (3 * C + U) + St + B * Sp * (Cin + C))
    b_step = 4 * N * (B * (4 * C + U) + St + B * Cin)
    Xo, Do = ours_train()
    Xt, Dt = torch_train()
    e_train = ((Xo - Xt).abs().max().item(), (Do - Dt).abs().max().item())
    e_step = (ours_step() - torch_step()).abs().max().item()
    del Xo, Do, Xt, Dt
    n_train, n_step = counted(torch_train), counted(torch_step)
    for label, ours, composed, nbytes, nops, err in (("training assemble S'=4", ours_train, torch_train, b_train, n_train, e_train),
                                                     ("sampler step (Foellmer)", ours_step, torch_step, b_step, n_step, e_step)):
        for rnd in range(3):
            t, tt = timed(ours), timed(composed)
            print(f"interpolant {label:24s} round {rnd}: 1 launch {t:7.3f} ms = {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s = "
                  f"{nbytes / (t * 1e-3) / PEAK * 100:5.1f} % of the HBM roof ({nbytes / 1e9:.2f} GB) | torch sequence, {nops} compute ops, "
                  f"{tt:7.3f} ms = {nbytes / (tt * 1e-3) / 1e12:5.2f} TB/s of the same bytes = {tt / t:5.2f} x | max |kernel - torch| {err}",
                  flush=True)


def losshandler():
    """What LossHandler adds (csrc/hydro.hip) at (B, E, C, H, W) = (1, 16, 73, 721, 1440), bf16: the moist hydrostatic loss on 13
    levels, forward + backward on the (1, 73, 721, 1440) ensemble mean, and the preparation launch with all four outputs (mean,
    member tendencies, mean tendency, target tendency); each beside the same steps written in torch on the same tensors in the same
    process (the reference's formulation: .float(), scale and bias, the moist correction, the matmul with cmat, square, quadrature,
    backward by autograd; torch.mean and three subtractions), timed in turn over three rounds.  Algorithmic bytes: hydrostatic
    one read of the 39 channels it uses per direction plus one write of all 73 in the backward; preparation one read of the members,
    the target and the input state, one write of the four outputs."""
    H, W, B, E = 721, 1440, 1, 16
    N = H * W
    levels = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
    names = ["u10m", "v10m", "u100m", "v100m", "t2m", "sp", "msl", "tcwv"] + [f"{v}{p}" for v in "uvztq" for p in levels]
    C = len(names)
    gen = torch.Generator().manual_seed(1)
    bias, scale = torch.zeros(1, C, 1, 1), torch.ones(1, C, 1, 1)
    for i, n in enumerate(names):
        if n[1:].isdigit():
            k = math.log(1000.0 / int(n[1:])) / math.log(20.0)
            b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3), "t": (285.0 - 70.0 * k, 15.0), "q": (2.0e-3, 2.0e-3), "u": (5.0, 10.0), "v": (0.0, 8.0)}[n[0]]
            bias[0, i], scale[0, i] = b, s
    PEAK, dt = 8.0e12, torch.bfloat16

    def timed(fn):
        once = max(timeit(fn, reps=3, warm=2), 1e-3)
        return timeit(fn, reps=max(5, int(math.ceil(500.0 / once))), warm=1)

    m = ma.HydrostaticBalanceLoss((H, W), (H, W), (0, 0), names, "equiangular", bias, scale, p_min=50, p_max=1000, use_moist_air_formula=True).to(dev)
    x = torch.randn(B, C, H, W, generator=gen).to(dt).to(dev).requires_grad_(True)
    g = torch.randn(B, len(levels) - 1, generator=gen).to(dev)
    q = m.quadrature.quad_weight

    def torch_hydro(x):
        u = x.to(torch.float32) * m.scale + m.bias
        u[:, m.t_idx] = u[:, m.t_idx] * (1.0 + m.q_prefact * u[:, m.q_idx])
        r = torch.matmul(m.cmat, u.permute(1, 0, 2, 3).reshape(C, -1)).reshape(-1, B, H, W).permute(1, 0, 2, 3)
        return torch.sum(torch.square(r) * q, dim=(-2, -1)).to(x.dtype)

    ours = lambda: torch.autograd.grad(m(x, None), x, g.to(dt))[0]          # noqa: E731
    composed = lambda: torch.autograd.grad(torch_hydro(x), x, g.to(dt))[0]          # noqa: E731
    err = ((m(x, None).float() - torch_hydro(x).float()).abs().max().item() / torch_hydro(x).float().abs().max().item(),
           (ours().float() - composed().float()).abs().max().item() / composed().float().abs().max().item())
    nbytes = (2 * 39 + C) * B * N * 2
    for rnd in range(3):
        t, tt = timed(ours), timed(composed)
        print(f"losshandler hydrostatic moist bf16 round {rnd}: forward + backward {t:7.3f} ms = {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s = "
              f"{nbytes / (t * 1e-3) / PEAK * 100:5.1f} % of the HBM roof ({nbytes / 1e9:.2f} GB) | torch formulation {tt:7.3f} ms = {tt / t:5.2f} x | "
              f"max |kernel - torch| / max {err[0]:.1e} {err[1]:.1e}", flush=True)
    del x

    prd = torch.randn(B, E, C, H, W, generator=gen).to(dt).to(dev)
    tar, hist = torch.randn(B, C, H, W, generator=gen).to(dt).to(dev), torch.randn(B, 2 * C, H, W, generator=gen).to(dt).to(dev)
    inp = hist[:, -C:]
    flags = ops.PREP_MEAN | ops.PREP_MEMBER_T | ops.PREP_MEAN_T | ops.PREP_TAR_T

    def ours_prep():
        return ops.loss_prep_launch(prd, tar, inp, flags, 1.0 / E)

    def torch_prep():
        prdm = torch.mean(prd, dim=1)
        return prdm, prd - inp.unsqueeze(1), prdm - inp, tar - inp

    a, b = ours_prep(), torch_prep()
    err = [(u.float() - v.float()).abs().max().item() for u, v in zip(a, b)]
    del a, b
    nbytes = ((E + 2) + (E + 3)) * B * C * N * 2
    for rnd in range(3):
        t, tt = timed(ours_prep), timed(torch_prep)
        print(f"losshandler preparation E={E} bf16 all four outputs round {rnd}: {t:7.3f} ms = {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s = "
              f"{nbytes / (t * 1e-3) / PEAK * 100:5.1f} % of the HBM roof ({nbytes / 1e9:.2f} GB) | torch (mean and three subtractions) {tt:7.3f} ms = "
              f"{tt / t:5.2f} x | max |kernel - torch| {' '.join(f'{e:.1e}' for e in err)}", flush=True)


def mhandler():
    """One fused ``MetricsHandler.update`` (csrc/mrollout.hip: mk_mrollout_sums + mk_mrollout_finish) beside the composed
    per-handle path (``use_fused = False``: the ensemble mean, a gathered copy per handle, the NaN test with its host read, one
    metric pass per handle on csrc/metrics.hip and csrc/crps.hip, stack / combine / copy_) on the same GPU, in the same process,
    the two timed in turn over three rounds.  Shapes: (1, 16, 73, 721, 1440) bf16 and (1, 1, 73, 721, 1440) f32 with the eight
    default variables.  Each time as a share of the HBM roof for ITS OWN algorithmic traffic: fused = the (E + 1) * 8 selected
    planes, the quadrature weights and ACC's climatology once; composed = the mean over all C channels (read E C planes, write
    C fp32), and per handle the gathered copies of prediction and target (read + write), the NaN test (read) and the metric's
    own read of both (+ the climatology for ACC)."""
    PEAK = 8.0e12
    H, W, C, B = 721, 1440, 73, 1
    N = H * W
    names = ["u10m", "t2m", "sp", "sst", "u500", "z500", "q500", "q50"] + [f"x{i}" for i in range(C - 8)]

    class P(dict):
        __getattr__ = dict.__getitem__

    rate = lambda nbytes, ms: f"{nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s = {nbytes / (ms * 1e-3) / PEAK * 100:5.1f} % of the HBM roof"
    with torch.no_grad():
        clim = torch.randn(1, C, H, W)
        for E, dt in ((16, torch.bfloat16), (1, torch.float32)):
            s = 2 if dt == torch.bfloat16 else 4
            params = P(channel_names=names, dt=1, dhours=6, img_shape_x_resampled=H, img_shape_y_resampled=W, ensemble_size=E)
            kw = {} if E > 1 else dict(crps_var_names=[], spread_var_names=[], ssr_var_names=[])
            h = ma.MetricsHandler(params, clim, 4, dev, **kw)
            h.initialize_buffers()
            h.zero_buffers()
            prd = torch.randn((B, E, C, H, W) if E > 1 else (B, C, H, W), device=dev).to(dt)
            tar = (prd.float().mean(dim=1) if E > 1 else prd.float()) + torch.randn(B, C, H, W, device=dev)
            tar = tar.to(dt)
            loss = torch.zeros((), device=dev)
            J, nh = 8, len(h.metric_handles)
            ndet, nens = 3, nh - 3
            fused_bytes = ((E + 1) * J * s + 4 + J * 4) * N
            comp_bytes = ((E * C * s + C * 4) if E > 1 else 0) * N
            comp_bytes += ndet * (2 * J * 4 + 2 * J * s + J * s + J * 4 + J * s) * N + J * 4 * N          # + ACC's climatology
            comp_bytes += nens * (2 * E * J * s + 2 * J * s + J * s + (E + 1) * J * s) * N

            def run(fused):
                h.use_fused = fused
                h.update(prd, tar, loss, 1)

            for rnd in range(3):
                tf, tc = timeit(lambda: run(True), reps=20, warm=3), timeit(lambda: run(False), reps=5, warm=2)
                print(f"mhandler E={E:2d} {str(dt)[6:]} {nh} handles round {rnd}: fused {tf:7.3f} ms {rate(fused_bytes, tf)} ({fused_bytes / 1e9:.2f} GB)"
                      f" | composed {tc:8.3f} ms {rate(comp_bytes, tc)} ({comp_bytes / 1e9:.2f} GB) = {tc / tf:5.1f} x", flush=True)
            del prd, tar, h


def fcn31():
    """The two full-grid stages of FourCastNet3.1 (csrc/impute.hip) at 721 x 1440, B = 1, forward + backward, f32 and bf16: the
    SST imputation on 150 input channels (one imputed channel, 2 hidden units, the land mask read from a channel of x, about 30 %
    of the pixels masked) and the output tail on 73 channels (skip from a 76-channel input, soft clamp with offsets on 14 water
    channels); each beside the reference's composition in plain torch (slice, isnan, where, scatter, two
    1x1 convolutions, where, scatter; gather, add, gather, clamp, index_copy; backward by autograd) on the same tensors in the
    same process, the two timed in turn over two rounds, every timing over a window of at least 0.5 s.  Algorithmic bytes: the
    imputation reads x and writes y, then reads x and g and writes gx (5 tensors); the tail reads d and the 73 skip planes and
    writes y, then reads g (and d, xin on the water channels) and writes gd and the full input gradient."""
    import types
    import torch.nn.functional as F
    from makani_amd.imputation import MLPImputation

    def compose_mlp(x, imp, mask, w1, b1, w2):
        idx = torch.as_tensor(imp, device=x.device)
        x_sub = x[:, idx]
        m = torch.logical_or(mask, torch.isnan(x_sub))
        x_zeroed = torch.where(m, torch.zeros_like(x_sub), x_sub)
        index = idx.view(1, -1, 1, 1).expand_as(x_zeroed)
        x_clean = x.scatter(1, index, x_zeroed)
        o = F.conv2d(F.gelu(F.conv2d(x_clean, w1[:, :, None, None], b1)), w2[:, :, None, None])
        return x_clean.scatter(1, index, torch.where(m, o, x_zeroed))

    def compose_tail(d, xin, pred, water, off):
        x = d + xin[:, torch.as_tensor(pred, device=d.device)]
        wi = torch.as_tensor(water, device=d.device)
        o = off.view(1, -1, 1, 1).to(x.dtype)
        t = x[:, wi] + o
        y = torch.where(t > 0.0, t ** 2, 0.0)
        return x.index_copy(1, wi, (torch.where(t >= 0.5, t - 0.25, y) - o).to(x.dtype))

    ref = types.SimpleNamespace(compose_mlp=compose_mlp, compose_tail=compose_tail)
    PEAK = 8.0e12
    H, W, B = 721, 1440, 1
    N = H * W
    gen = torch.Generator().manual_seed(1)

    def timed(fn):
        once = max(timeit(fn, reps=3, warm=2), 1e-3)
        return timeit(fn, reps=max(5, int(math.ceil(500.0 / once))), warm=1)

    def report(label, dt, nbytes, ours, composed, err):
        for rnd in range(2):
            t, tt = timed(ours), timed(composed)
            print(f"fcn31 {label:10s} {str(dt)[6:]:8s} round {rnd}: forward + backward {t:7.3f} ms = {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s "
                  f"= {nbytes / (t * 1e-3) / PEAK * 100:5.1f} % of the HBM roof ({nbytes / 1e9:.2f} GB) | torch composition {tt:7.3f} ms = "
                  f"{tt / t:5.2f} x | max |kernel - torch| {err[0]:.1e} {err[1]:.1e}", flush=True)

    C, SST, LSM = 150, 4, 148
    mod = MLPImputation(C, torch.tensor([SST]), 2.0, mask_channel=LSM).to(dev)
    p = [mod.mlp.fwd[0].weight, mod.mlp.fwd[0].bias, mod.mlp.fwd[2].weight]
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(B, C, H, W, generator=gen)
        u = torch.rand(B, H, W, generator=gen)
        x[:, LSM] = torch.where(u < 0.7, torch.zeros(()), (u - 0.7) / 0.3)
        x[:, SST] = torch.where(x[:, LSM] != 0, torch.full((), float("nan")), x[:, SST])
        x = x.to(dt).to(dev).requires_grad_(True)
        g = torch.randn(B, C, H, W, generator=gen).to(dt).to(dev)
        w = [t.detach().view(t.shape[:2]).to(dt) if t.dim() == 4 else t.detach().to(dt) for t in p]
        w = [t.requires_grad_(True) for t in w]

        def ours():
            return torch.autograd.grad(mod(x), [x] + p, g)[0]

        def composed():
            return torch.autograd.grad(ref.compose_mlp(x, [SST], (x[:, LSM] != 0)[:, None], *w), [x] + w, g)[0]

        err = ((mod(x).detach().float() - ref.compose_mlp(x, [SST], (x[:, LSM] != 0)[:, None], *w).detach().float()).abs().max().item(),
               (ours().float() - composed().float()).abs().max().item())
        report("imputation", dt, 5 * C * B * N * x.element_size(), ours, composed, err)
        del x, g

    Co, Cin = 73, 76
    water = [7] + list(range(60, 73))
    pred = list(range(8)) + list(range(11, 76))
    off = torch.linspace(0.2, 1.5, len(water))
    table = ops.tail_table(Co, water, off, pred, Cin, dev)
    for dt in (torch.float32, torch.bfloat16):
        d = torch.randn(B, Co, H, W, generator=gen).to(dt).to(dev).requires_grad_(True)
        xin = torch.randn(B, Cin, H, W, generator=gen).to(dt).to(dev).requires_grad_(True)
        g = torch.randn(B, Co, H, W, generator=gen).to(dt).to(dev)
        offd = off.to(dev)
        nbytes = (3 * Co + Co + 2 * len(water) + Co + Cin) * B * N * d.element_size()

        def ours():
            return torch.autograd.grad(ops.Fcn31TailFn.apply(d, xin, table), [d, xin], g)

        def composed():
            return torch.autograd.grad(ref.compose_tail(d, xin, pred, water, offd), [d, xin], g)

        err = ((ours()[0].float() - composed()[0].float()).abs().max().item(), (ours()[1].float() - composed()[1].float()).abs().max().item())
        report("tail", dt, nbytes, ours, composed, err)
        del d, xin, g


if __name__ == "__main__":
    which = sys.argv[1:] or ["fft", "legendre", "dhconv", "pointwise"]
    for w in which:
        globals()[w]()
