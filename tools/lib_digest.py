"""SHA-256 of every output of the kernels that share csrc/block_io.h, on fixed inputs at small shapes, from whichever library
MAKANI_AMD_LIB names.  Two builds whose arithmetic and summation orders agree print the same lines:
       python tools/ab.py run parent new -- python tools/lib_digest.py
   python tools/lib_digest.py [crps] [nll] [metrics] [escore] [egram] [preproc] [layernorm] [resample] [disco] [optim] [losshandler]
Shapes: 33 x 40 points (a multiple of 4, two chunks of a plane) and 33 x 41 (odd: one element per thread), bases aligned and
shifted by one element, both element types, ensembles of 2, 3, 5, 9 and 17 (every compiled capacity, each partly filled)."""
import ctypes as C
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from makani_amd import _lib, disco as mdisco
from makani_amd._lib import lib, ptr, stream, check, dtype_code

dev = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
ES = (2, 3, 5, 9, 17)
gen = torch.Generator().manual_seed(20250)


def rnd(*shape, dt=F32, shift=0, scale=1.0, pos=False):
    """seeded values made on the host; shift = 1: the tensor starts one element behind an aligned base"""
    v = torch.rand(*shape, generator=gen) + 0.5 if pos else torch.randn(*shape, generator=gen) * scale
    buf = torch.empty(v.numel() + shift, dtype=dt, device=dev)
    buf[shift:] = v.flatten().to(dev).to(dt)
    return buf[shift:].view(*shape)


def emit(name, *outs):
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        raw = (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.uint8).cpu().numpy().tobytes()
        print(f"{name} [{i}] {hashlib.sha256(raw).hexdigest()}", flush=True)


def tag(t):
    return "bf16" if t == BF16 else "f32"


def crps():
    B, C, hw = 2, 3, 33 * 40
    q, w, gout, ew = rnd(hw, pos=True), rnd(B, C, hw, pos=True), rnd(B * C), rnd(17, pos=True)
    ch = lib().mk_crps_chunks(hw)
    for E in ES:
        for df, do in ((F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16)):
            f, o = rnd(B, E, C, hw, dt=df), rnd(B, C, hw, dt=do)
            for typ in range(5):
                part, gf = torch.zeros(B * C, ch, device=dev), torch.zeros_like(f)
                for grad in (0, 1):
                    check(lib().mk_crps(ptr(f), dtype_code(f), ptr(o), dtype_code(o), ptr(q), ptr(w) if typ % 2 else None, ptr(gout), ptr(part),
                                        ptr(gf), B, E, C, hw, typ, 0.9, 1e-5, grad, ptr(ew) if typ == 4 else None, stream()))
                emit(f"crps E={E} {tag(df)}/{tag(do)} type={typ}", part, gf)
        f = torch.view_as_complex(rnd(B, E, C, hw, 2))
        o = torch.view_as_complex(rnd(B, C, hw, 2))
        part, gf = torch.zeros(B * C, ch, device=dev), torch.zeros_like(f)
        for grad in (0, 1):
            check(lib().mk_crps_complex(ptr(f), ptr(o), ptr(q), ptr(w), ptr(gout), ptr(part), ptr(gf), B, E, C, hw, 0.9, grad, stream()))
        emit(f"crps_complex E={E}", part, gf)


def egram():
    B, C, L, M = 2, 3, 5, 70
    q = rnd(L, M, pos=True)
    for E in (1,) + ES + (32,):
        f, o = torch.view_as_complex(rnd(B, E, C, L, M, 2)), torch.view_as_complex(rnd(B, C, L, M, 2))
        for what, K in ((0, E + 1), (1, 2 * E + 1), (2, 2 * E + 1 + E * (E - 1) // 2)):
            for tri_off in (0, M):
                G, dG, gf = torch.zeros(B, C, L, K, device=dev), rnd(B, C, L, K), torch.zeros_like(f)
                check(lib().mk_egram_sums(ptr(f), ptr(o), ptr(q), ptr(G), B, E, C, L, M, what, tri_off, stream()))
                check(lib().mk_egram_grad(ptr(f), ptr(o), ptr(q), ptr(dG), ptr(gf), B, E, C, L, M, what, tri_off, stream()))
                emit(f"egram E={E} what={what} tri_off={tri_off}", G, gf)


def nll():
    B, C, hw = 2, 3, 33 * 40
    q, w, gout = rnd(hw, pos=True), rnd(B, C, hw, pos=True), rnd(B * C)
    ch = lib().mk_ens_nll_chunks(hw)
    for E in (1,) + ES:
        for df in (F32, BF16):
            f, o = rnd(B, E, C, hw, dt=df), rnd(B, C, hw)
            part, gf = torch.zeros(B * C, ch, device=dev), torch.zeros_like(f)
            for grad in (0, 1):
                check(lib().mk_ens_nll(ptr(f), dtype_code(f), ptr(o), ptr(q), ptr(w) if E % 2 else None, ptr(gout), ptr(part), ptr(gf), B, E, C,
                                       hw, 1e-3, grad, stream()))
            emit(f"ens_nll E={E} {tag(df)}", part, gf)


def metrics():
    B, C = 2, 3
    for n, shift in ((33 * 40, 0), (33 * 40, 1), (33 * 41, 0)):
        ch = lib().mk_metric_chunks(n)
        q, w, bias = rnd(n, pos=True), rnd(B, C, n, pos=True), rnd(C, n)
        for dx, dy in ((F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16)):
            x, y = rnd(B, C, n, dt=dx, shift=shift), rnd(B, C, n, dt=dy)
            for which, b_, w_ in ((31, bias, w), (2, None, None), (5, bias, None)):
                out, ws = torch.zeros(B, C, 5, device=dev), torch.zeros(B * C * ch * 5, device=dev)
                check(lib().mk_metric_det_sums(ptr(x), dtype_code(x), ptr(y), dtype_code(y), ptr(b_), ptr(w_), ptr(q), ptr(out), ptr(ws), B, C,
                                               n, which, stream()))
                emit(f"metric_det n={n} shift={shift} {tag(dx)}/{tag(dy)} which={which}", out)
        for E in (1,) + ES:
            for df in (F32, BF16):
                f, o = rnd(B, E, C, n, dt=df, shift=shift), rnd(B, C, n)
                for which, w_ in ((7, w), (3, None), (4, None)):
                    out, ws = torch.zeros(B, C, E + 3, device=dev), torch.zeros(B * C * ch * (E + 3), device=dev)
                    check(lib().mk_metric_ens_sums(ptr(f), dtype_code(f), ptr(o), ptr(w_), ptr(q), ptr(out), ptr(ws), B, E, C, n, which, stream()))
                    emit(f"metric_ens n={n} shift={shift} E={E} {tag(df)} which={which}", out)


def escore():
    B, C, N = 2, 3, 33 * 40
    q, w = rnd(N, pos=True) / N, rnd(B, C, N, pos=True)
    for E in (1,) + ES:
        K = E + E * (E - 1) // 2
        for kind, p, S, nanmode in ((0, 2.0, 1, 0), (0, 1.0, 1, 0), (0, 1.5, 1, 0), (1, 2.0, 1, 0), (1, 1.0, 33, 1), (2, 2.0, 33, 1)):
            if kind == 2:
                f, o = torch.view_as_complex(rnd(B, E, C, N, 2)), torch.view_as_complex(rnd(B, C, N, 2))
            else:
                f, o = rnd(B, E, C, N, dt=BF16 if kind else F32), rnd(B, C, N)
            sums = torch.zeros(B, C, S, K, device=dev)
            ws = torch.zeros(max(1, lib().mk_escore_sums_workspace(B, E, C, N, S, nanmode)), device=dev)
            check(lib().mk_escore_sums(ptr(f), kind, ptr(o), ptr(q), ptr(w), ptr(sums), ptr(ws), B, E, C, N, S, nanmode, p, stream()))
            for reduce in (0, 1):
                Co = 1 if reduce else C
                loss, table, gout, gf = torch.zeros(B, Co, device=dev), torch.zeros(B, Co, S, K, device=dev), rnd(B, Co), torch.zeros_like(f)
                check(lib().mk_escore_finish(ptr(sums), None, 0, ptr(loss), ptr(table), B, E, C, S, reduce, p, 1.0, 0.9, 1e-12, stream()))
                check(lib().mk_escore_grad(ptr(f), kind, ptr(o), ptr(q), ptr(w), ptr(table), ptr(gout), ptr(gf), B, E, C, Co, N, S, nanmode, p,
                                           stream()))
                emit(f"escore E={E} kind={kind} p={p} S={S} reduce={reduce}", sums, loss, table, gf)
            if S == 1:
                loss, table = torch.zeros(B, C, device=dev), torch.zeros(B, C, 1, K, device=dev)
                check(lib().mk_mmd_finish(ptr(sums), ptr(loss), ptr(table), B, E, C, 0, 4.0, 0.9, stream()))
                emit(f"mmd_finish E={E} kind={kind} p={p}", loss, table)


def preproc():
    B, T, C, U, N, S = 2, 2, 3, 1, 2, 2
    J = C + U + N
    for hw, shift in ((2112, 0), (2112, 1), (2113, 0), (8196, 0)):          # 2112: two streaming chunks; 8196: two reduction chunks
        ch = lib().mk_prep_chunks(hw)
        q, wt = rnd(hw, pos=True) / hw, torch.full((T,), 1.0 / T, device=dev)
        for dt in (F32, BF16):
            win, unp, noi = rnd(B, T * C, hw, dt=dt, shift=shift, scale=2.0), rnd(B, T, U, hw, dt=dt), rnd(B, T, N, hw, dt=dt)
            stat, bias, yn, gyn = rnd(S, hw, dt=dt), rnd(C, hw), rnd(B, C, hw, dt=dt), rnd(B, C, hw, dt=dt)
            g = rnd(B, T * J + S, hw, dt=dt)
            src = (ptr(win), dtype_code(win), ptr(unp), dtype_code(unp), ptr(noi), dtype_code(noi))
            dims = (B, T, T * C, U, N)
            mu, sigma, tri = torch.zeros(B, J, device=dev), torch.zeros(B, J, device=dev), torch.zeros(B, J, 3, dtype=torch.float64, device=dev)
            ws = torch.zeros(B * J * ch * 4, device=dev)
            check(lib().mk_prep_stats(*src, ptr(q), ptr(wt), ptr(mu), ptr(sigma), ptr(tri), ptr(ws), *dims, hw, stream()))
            out, y = torch.zeros(B, T * J + S, hw, dtype=dt, device=dev), torch.zeros_like(yn)
            check(lib().mk_prep_assemble(*src, ptr(stat), dtype_code(stat), ptr(mu), ptr(sigma), ptr(out), dtype_code(out), *dims, S, hw, stream()))
            check(lib().mk_prep_finish(ptr(yn), dtype_code(yn), ptr(bias), ptr(mu), ptr(sigma), ptr(y), B, C, J, hw, stream()))
            G, gmu, gsig = torch.zeros(2, B, J, device=dev), rnd(B, J), rnd(B, J)
            check(lib().mk_prep_bwd_sums(ptr(g), dtype_code(g), *src, ptr(mu), ptr(sigma), ptr(gmu), ptr(gsig), ptr(G), ptr(ws), *dims, S, 3, hw,
                                         stream()))
            dwin, dnoi = torch.zeros_like(win), torch.zeros_like(noi)
            check(lib().mk_prep_bwd_apply(ptr(g), dtype_code(g), *src, ptr(q), ptr(wt), ptr(mu), ptr(sigma), ptr(G), ptr(dwin), ptr(dnoi), *dims, S,
                                          hw, stream()))
            fmu, fsig = torch.zeros(B, J, device=dev), torch.zeros(B, J, device=dev)
            check(lib().mk_prep_finish_bwd(ptr(gyn), dtype_code(gyn), ptr(yn), dtype_code(yn), ptr(bias), ptr(fmu), ptr(fsig), ptr(ws), B, C, J, hw,
                                           stream()))
            emit(f"preproc hw={hw} shift={shift} {tag(dt)}", mu, sigma, tri, out, y, G, dwin, dnoi, fmu, fsig)


def layernorm():
    B, C = 2, 5
    gamma, beta = rnd(C), rnd(C)
    for P in (63, 64):
        ch = lib().mk_chan_layernorm_chunks(C, P)
        for dx, dy in ((F32, F32), (BF16, F32), (BF16, BF16)):
            x, gy = rnd(B, C, P, dt=dx, scale=3.0), rnd(B, C, P, dt=dy)
            y, stats = torch.zeros(B, C, P, dtype=dy, device=dev), torch.zeros(B, 2, P, device=dev)
            gx, part = torch.zeros_like(x), torch.zeros(2, C, ch, device=dev)
            check(lib().mk_chan_layernorm_fwd(ptr(x), dtype_code(x), ptr(y), dtype_code(y), ptr(stats), ptr(gamma), ptr(beta), B, C, P, 1e-5,
                                              stream()))
            check(lib().mk_chan_layernorm_bwd(ptr(x), dtype_code(x), ptr(gy), dtype_code(gy), ptr(gx), ptr(stats), ptr(gamma), B, C, P, stream()))
            check(lib().mk_chan_layernorm_wgrad(ptr(x), dtype_code(x), ptr(gy), dtype_code(gy), ptr(stats), ptr(part), B, C, P, stream()))
            emit(f"chan_layernorm P={P} {tag(dx)}/{tag(dy)}", y, stats, gx, part)


def resample():
    # Gauss rows to an equiangular grid that reaches both poles: the first and last output rows read the polar means
    m = mdisco.ResampleS2(8, 16, 17, 40, grid_in="legendre-gauss", grid_out="equiangular").to(dev)
    assert m.expand_poles
    for dt in (F32, BF16):
        x, gy = rnd(3, 8, 16, dt=dt), rnd(3, 17, 40, dt=dt)
        emit(f"resample {tag(dt)}", m._launch(x, False), m._launch(gy, True))


def disco():
    for out_shape in ((12, 24), (6, 12)):          # equal longitudes: mk_disco_bwd_same; otherwise the gather of mk_disco_bwd
        m = mdisco.DiscreteContinuousConvS2(1, 1, (12, 24), out_shape, (2, 2), bias=False)
        L = m._device_lists(dev)
        planes, (hi, wi), (ho, wo) = 3, L.in_shape, L.out_shape
        for dt in (F32, BF16):
            x, gy = rnd(planes, hi, wi, dt=dt), rnd(planes * L.K, ho, wo, dt=dt)
            y, gx = torch.zeros(planes * L.K, ho, wo, dtype=dt, device=dev), torch.zeros_like(x)
            check(lib().mk_disco_fwd(ptr(x), ptr(y), dtype_code(x), ptr(L.f_off), ptr(L.f_row), ptr(L.f_lon), ptr(L.f_val), ptr(L.lat_lo),
                                     ptr(L.lat_n), L.max_rows, planes, L.K, hi, wi, ho, wo, stream()))
            if L.same_lon:
                check(lib().mk_disco_bwd_same(ptr(gy), ptr(gx), dtype_code(gy), ptr(L.s_off), ptr(L.s_row), ptr(L.s_lon), ptr(L.s_val), ptr(L.t_lo),
                                              ptr(L.t_n), L.max_rows_b, planes, L.K, hi, wi, ho, stream()))
            else:
                check(lib().mk_disco_bwd(ptr(gy), ptr(gx), dtype_code(gy), ptr(L.b_off), ptr(L.b_k), ptr(L.b_t), ptr(L.b_lon), ptr(L.b_val), planes,
                                         L.K, hi, wi, ho, wo, stream()))
            emit(f"disco {hi}x{wi}->{ho}x{wo} {tag(dt)}", y, gx)


def optim():
    from makani_amd.optim import _k_sumsq_clip
    n = 40003                                                   # three blocks of the sum of squares, a tail that is no multiple of 4
    g, gs, pre = rnd(n), rnd(n, shift=1), rnd(700, pos=True)    # 16-byte aligned, shifted by one element, producers' partial sums
    emit("grad_clip_coef aligned", _k_sumsq_clip([g], 1.0))
    emit("grad_clip_coef shifted", _k_sumsq_clip([gs], 1.0))
    emit("grad_clip_coef both + partials", _k_sumsq_clip([g, gs], 0.5, pre=[pre]))
    p, m, v = rnd(n), rnd(n, scale=0.1), rnd(n, pos=True)
    st = torch.zeros(3, device=dev)
    check(lib().mk_adamw_advance(ptr(st), 0.9, 0.999, stream()))
    check(lib().mk_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), n, None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, ptr(st), stream()))
    emit("adamw_step", st, p, m, v)
    p2, m2, v2 = rnd(n), rnd(n, scale=0.1), rnd(n, pos=True)
    desc = (_lib.MkAdamTensor * 1)(_lib.MkAdamTensor(p2.data_ptr(), g.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, None, None, 0, 0, 0))
    check(lib().mk_adamw_multi(desc, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, ptr(st), stream()))
    emit("adamw_multi", p2, m2, v2)


def losshandler():
    B, C, K = 2, 9, 3                                           # z, t, q on three levels: channels 0 .. 8 in that order
    ftab = torch.cat([rnd(16, pos=True) for _ in range(7)])
    for n, shift in ((33 * 40, 0), (33 * 40, 1), (33 * 41, 0), (70 * 1024, 0)):          # the last: more points than 64 chunks of 1024
        ch = lib().mk_hydro_chunks(n)
        q, w, gout = rnd(n, pos=True) / n, rnd(B, K - 1, n, pos=True), rnd(B, K - 1)
        for moist in (0, 1):
            idx = [0, 1, 2] + [2] * 13 + [3, 4, 5] + [5] * 13 + ([6, 7, 8] + [8] * 13 if moist else [0] * 16) + ([] if moist else [6, 7, 8])
            itab = torch.tensor(idx, dtype=torch.int32, device=dev)
            for dt in (F32, BF16):
                x = rnd(B, C, n, dt=dt, shift=shift)
                out, ws, gx = torch.zeros(B, K - 1, device=dev), torch.zeros(B * (K - 1) * ch, device=dev), torch.zeros_like(x)
                tail = (ptr(itab), ptr(ftab), B, C, K, K if moist else 0, 0 if moist else 3, 0.6078, n, stream())
                check(lib().mk_hydro_sums(ptr(x), dtype_code(x), ptr(w), (K - 1) * n, n, ptr(q), ptr(out), ptr(ws), *tail))
                check(lib().mk_hydro_grad(ptr(x), dtype_code(x), ptr(w), (K - 1) * n, n, ptr(q), ptr(gout), ptr(gx), *tail))
                emit(f"hydro n={n} shift={shift} moist={moist} {tag(dt)}", out, gx)
    for n, shift in ((2112, 0), (2112, 1), (2113, 0)):
        for E in (1,) + ES + (32,):
            for dt in (F32, BF16):
                prd, tar, inp = rnd(B, E, n, dt=dt, shift=shift), rnd(B, n, dt=dt), rnd(B, n, dt=dt)
                outs = [torch.zeros(B, n, dtype=dt, device=dev), torch.zeros_like(prd), torch.zeros(B, n, dtype=dt, device=dev), torch.zeros(B, n, dtype=dt, device=dev)]
                check(lib().mk_loss_prep_fwd(ptr(prd), ptr(tar), ptr(inp), n, dtype_code(prd), *(ptr(o) for o in outs), 15, 1.0 / E, B, E, n, stream()))
                g = torch.zeros_like(prd)
                check(lib().mk_loss_prep_bwd(ptr(outs[1]), ptr(outs[0]), ptr(outs[2]), ptr(g), dtype_code(g), 1.0 / E, B, E, n, stream()))
                emit(f"loss_prep n={n} shift={shift} E={E} {tag(dt)}", *outs, g)


if __name__ == "__main__":
    print(f"library {_lib.LIB_PATH}", file=sys.stderr)
    for fam in sys.argv[1:] or ["crps", "nll", "metrics", "escore", "egram", "preproc", "layernorm", "resample", "disco", "optim", "losshandler"]:
        globals()[fam]()
