"""The plane sums of the geometric validation metrics on the GPU (csrc/metrics.hip, makani_amd/metrics.py) against the fp64
restatement of tests/_metrics_ref.py: <= 1e-5 relative L2 per output (the gate of the loss kernels); rank
histogram bins one by one, per (b, c) entry: relative error <= 1e-5 where the bin is occupied, exactly 0 where it is empty.

Shapes: B = 2, C = 3 on 17 x 32 (N = 544: one chunk, 16-byte path), 9 x 14 (N = 126, not a multiple of 4: one point per thread
and a tail) and 91 x 180 (N = 16 380: 16 chunks per plane, a partial last block); E = 1, 2, 3, 8, 9, 32 (every compiled capacity
2, 4, 8, 16, 32; 32 members always take the one-point path); fp32 and bf16 members (the restatement scores the bf16-rounded
values), all four dtype pairs of x and y, with and without weight and bias.

The inputs are conditioned so that 1e-5 tests the kernels and not cancellation; the reference FORMULA in plain fp32 torch on the
CPU (functions.py's own sequence: differences, sort + searchsorted(side="right") + one_hot) meets the same gate against the
restatement on them — test_inputs_let_the_fp32_formula_meet_the_tolerance asserts it, no GPU needed:
  * deterministic: x and y share a field of std 3 and carry independent noise of std 1, the climatology is a smooth field of
    std 1: every one of the five sums is a sum of mostly same-signed terms (correlation of the anomalies about 0.9).
  * ensemble: members = a common field (std 3) + the offsets e - (E - 1) / 2 + bounded noise (|.| <= 0.35), as the likelihood
    test of tests/test_gpu_restloss.py: centred squares of order 1 and more.  Observations are spread uniformly over slightly
    more than the ensemble's range, so every bin is occupied on the large grid; on a sixteenth of the points each the
    observation EQUALS one member, equals two equal members, lies below all and above all members (bf16: equality with the
    rounded value, which the kernel sees).
fp32 torch formula against the restatement on these inputs, worst case over the cases (relative L2 per output; bins per entry):
  deterministic sums 8.6e-08,  skill 6.6e-08,  spread 7.4e-08,  occupied bins 1.6e-07 (empty bins exactly 0)."""
import pytest
import torch
import torch.nn.functional as F

import _metrics_ref as ref
from _ranks import launch, ranks
from conftest import load_golden

GRIDS = [(17, 32), (9, 14), (91, 180)]
B, C = 2, 3
ES = [1, 2, 3, 8, 9, 32]
TOL = 1e-5
f32, bf16 = torch.float32, torch.bfloat16

# (grid, x dtype, y dtype, weight, bias)
DET_CASES = ([(2, dx, dy, True, True) for dx in (f32, bf16) for dy in (f32, bf16)]
             + [(0, f32, f32, False, False), (0, f32, f32, True, True), (1, f32, f32, True, True), (1, bf16, bf16, True, False),
                (2, f32, f32, False, True)])
# (grid, E, member dtype, weight)
ENS_CASES = ([(2, E, f32, True) for E in ES] + [(2, 9, bf16, True), (2, 3, bf16, False)]
             + [(1, 1, f32, True), (1, 3, f32, False), (1, 32, f32, True), (1, 8, bf16, False)]
             + [(0, 2, f32, False), (0, 8, f32, True), (0, 16, bf16, True), (0, 32, f32, False)])


def _id(key):
    return "-".join(str(k).replace("torch.", "") for k in key)


def _kw(grid, **extra):
    return dict(grid_type="equiangular", img_shape=GRIDS[grid], crop_shape=GRIDS[grid], crop_offset=(0, 0), **extra)


def _smooth(n, gen, img):
    s = F.interpolate(torch.randn(n, 1, 4, 8, generator=gen), size=img, mode="bilinear", align_corners=True)
    return s.reshape(n, *img)


def det_inputs(key):
    grid, dx, dy, _, _ = key
    img = GRIDS[grid]
    gen = torch.Generator().manual_seed(100 + grid)
    common = 3.0 * torch.randn(B, C, *img, generator=gen)
    x = (common + torch.randn(B, C, *img, generator=gen)).to(dx)
    y = (common + torch.randn(B, C, *img, generator=gen)).to(dy)
    w = torch.rand(B, C, *img, generator=gen) + 0.5
    bias = _smooth(C, gen, img)
    return x, y, w, bias


def ens_inputs(key):
    grid, E, dt, _ = key
    img = GRIDS[grid]
    gen = torch.Generator().manual_seed(200 + 40 * grid + E)
    base = 3.0 * torch.randn(B, C, *img, generator=gen)
    f = (base.unsqueeze(1) + 0.7 * (torch.rand(B, E, C, *img, generator=gen) - 0.5)
         + (torch.arange(E) - 0.5 * (E - 1)).reshape(1, E, 1, 1, 1)).to(dt).float()          # the values the kernel sees
    o = base + 1.1 * (E + 1) * (torch.rand(B, C, *img, generator=gen) - 0.5)
    kind = (torch.arange(img[0] * img[1]) % 16).reshape(img)
    if E >= 2:
        f[:, 1] = torch.where(kind == 1, f[:, 0], f[:, 1])                  # two equal members ...
    o = torch.where(kind == 0, f[:, E // 2], o)                              # the observation equals one member,
    o = torch.where(kind == 1, f[:, 0], o)                                   # ... and the observation equals both,
    o = torch.where(kind == 2, f.min(dim=1).values - 1.0, o)                 # lies below all
    o = torch.where(kind == 3, f.max(dim=1).values + 1.0, o)                 # and above all members
    w = torch.rand(B, C, *img, generator=gen) + 0.5
    return f.to(dt), o, w


_REF = {}


def restatement(key):
    """the fp64 sums of a case, computed once per process: (B, C, 5) or (skill, centred squares, histogram)"""
    if key not in _REF:
        q = ref.quadrature_weights(GRIDS[key[0]])
        if len(key) == 5:
            x, y, w, bias = det_inputs(key)
            _REF[key] = ref.det_sums(x, y, q, w if key[3] else None, bias if key[4] else None)
        else:
            f, o, w = ens_inputs(key)
            _REF[key] = ref.ens_sums(f, o, q, w if key[3] else None)
    return _REF[key]


def bin_errors(hist, want):
    """(worst relative error over the occupied entries, whether every empty entry is exactly 0)"""
    hist, want = hist.detach().cpu().double(), want.double()
    assert hist.shape == want.shape
    occ = want > 0
    rel = ((hist[occ] - want[occ]).abs() / want[occ]).max().item() if bool(occ.any()) else 0.0
    return rel, bool((hist[~occ] == 0).all())


def _fp32_formula(key):
    """the reference's sequence of operations in plain fp32 torch on the CPU"""
    q = ref.quadrature_weights(GRIDS[key[0]]).float()
    if len(key) == 5:
        x, y, w, bias = det_inputs(key)
        x, y = x.float(), y.float()
        wt = q * w if key[3] else q
        a, b = (x - bias, y - bias) if key[4] else (x, y)
        terms = [torch.abs(x - y), torch.square(x - y), a * b, torch.square(a), torch.square(b)]
        return torch.stack([torch.sum(t * wt, dim=(-2, -1)) for t in terms], dim=-1)
    f, o, w = ens_inputs(key)
    f = f.float()
    E = f.shape[1]
    wt = (q * w if key[3] else q.expand(B, C, *q.shape))
    mean = torch.sum(f, dim=1) / float(E)
    skill = torch.sum(torch.square(mean - o) * wt, dim=(-2, -1))
    spread = torch.sum(torch.sum(torch.square(mean.unsqueeze(1) - f), dim=1) * wt, dim=(-2, -1))
    fs, _ = torch.sort(torch.moveaxis(f.flatten(3), 1, -1), dim=-1, descending=False, stable=True)
    ins = torch.searchsorted(fs.contiguous(), o.flatten(2).unsqueeze(-1).contiguous(), side="right").squeeze(-1)
    hist = torch.sum(F.one_hot(ins, num_classes=E + 1).to(torch.float32) * wt.flatten(2).unsqueeze(-1), dim=2)
    return skill, spread, hist


@pytest.mark.parametrize("key", DET_CASES + ENS_CASES, ids=_id)
def test_inputs_let_the_fp32_formula_meet_the_tolerance(key):
    """the conditioning of the inputs (module docstring), checked without the kernels"""
    want, got = restatement(key), _fp32_formula(key)
    if len(key) == 5:
        errs = [ref.mismatch(got[..., k], want[..., k]) for k in range(5)]
        print(f"{_id(key)}: fp32 torch formula vs fp64 restatement, the five sums {' '.join(f'{e:.2e}' for e in errs)}")
        assert max(errs) < TOL, errs
        return
    E = key[1]
    rel, zeros = bin_errors(got[2], want[2])
    errs = [ref.mismatch(got[0], want[0]), ref.mismatch(got[1], want[1]), rel]
    print(f"{_id(key)}: fp32 torch formula vs fp64 restatement, skill / spread / bins {' '.join(f'{e:.2e}' for e in errs)}")
    assert max(errs) < TOL and zeros, errs
    f, o, _ = ens_inputs(key)
    f = f.float()
    eq = (f == o.unsqueeze(1)).sum(dim=1)
    assert int((eq == 1).sum()) > 0 and int((f > o.unsqueeze(1)).all(dim=1).sum()) > 0 and int((f < o.unsqueeze(1)).all(dim=1).sum()) > 0
    if E >= 2:
        assert int((eq >= 2).sum()) > 0 and float(f.double().var(dim=1, correction=0).mean()) > 0.05
    if key[0] == 2 and E <= 9:
        assert float(want[2].min()) > 0          # every bin occupied on the large grid (E = 32: 33 bins, some (b, c) miss one)


def _q(grid, dev):
    import makani_amd as ma
    return ma.GridQuadrature("naive", GRIDS[grid]).to(dev)


def _det(key, dev, which, xs=None):
    import makani_amd as ma
    x, y, w, bias = det_inputs(key)
    x = xs if xs is not None else x.to(dev)
    return ma.deterministic_sums(x, y.to(dev), _q(key[0], dev), bias=bias.to(dev) if key[4] else None,
                                 weight=w.to(dev) if key[3] else None, which=which)


def _ens(key, dev, which, fs=None):
    from makani_amd import metrics as mm
    f, o, w = ens_inputs(key)
    img = GRIDS[key[0]]
    n = img[0] * img[1]
    f = fs if fs is not None else f.to(dev)
    q = _q(key[0], dev).quad_weight.reshape(-1)
    return mm._ens_launch(f.reshape(B, key[1], C, n), o.to(dev).reshape(B, C, n), q, w.to(dev).reshape(B, C, n) if key[3] else None, which)


@pytest.mark.gpu
@pytest.mark.parametrize("key", DET_CASES, ids=_id)
def test_deterministic_sums_match_the_restatement(key):
    dev = "cuda:0"
    want = restatement(key)
    out = _det(key, dev, 31)
    assert out.shape == (B, C, 5) and out.dtype == torch.float32
    errs = [ref.mismatch(out[..., k], want[..., k]) for k in range(5)]
    print(f"{_id(key)}: the five sums {' '.join(f'{e:.2e}' for e in errs)}")
    assert max(errs) < TOL, errs
    assert torch.equal(out, _det(key, dev, 31))                              # two calls: bit-identical
    # every mask a class uses and every single sum: the selected columns equal the all-at-once ones bit for bit, the others stay 0
    for which in (1, 2, 28, 4, 8, 16):
        part = _det(key, dev, which)
        for k in range(5):
            assert torch.equal(part[..., k], out[..., k] if which & (1 << k) else torch.zeros_like(out[..., k])), (which, k)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ENS_CASES, ids=_id)
def test_ensemble_sums_match_the_restatement(key):
    dev = "cuda:0"
    E = key[1]
    skill, ss, hist = restatement(key)
    out = _ens(key, dev, 7)
    assert out.shape == (B, C, E + 3) and out.dtype == torch.float32
    rel, zeros = bin_errors(out[..., 2:], hist)
    errs = [ref.mismatch(out[..., 0], skill), ref.mismatch(out[..., 1], ss), rel]
    print(f"{_id(key)}: skill / spread / bins {' '.join(f'{e:.2e}' for e in errs)}")
    assert max(errs) < TOL and zeros, errs
    assert torch.equal(out, _ens(key, dev, 7))                               # two calls: bit-identical
    for which in (2, 3, 4, 1):          # Spread, SSR, rank histogram, skill alone
        part = _ens(key, dev, which)
        sel = [which & 1, which & 2] + [which & 4] * (E + 1)
        for k in range(E + 3):
            assert torch.equal(part[..., k], out[..., k] if sel[k] else torch.zeros_like(out[..., k])), (which, k)


@pytest.mark.gpu
def test_a_base_that_is_not_16_byte_aligned_takes_the_scalar_path():
    """a slice that starts one float into an allocation: N = 544 would allow the 16-byte path, the pointer does not"""
    dev = "cuda:0"
    key = (0, f32, f32, True, True)
    x = det_inputs(key)[0]
    buf = torch.zeros(x.numel() + 1, device=dev)
    buf[1:] = x.reshape(-1).to(dev)
    xs = buf[1:].view(x.shape)
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    want = restatement(key)
    out = _det(key, dev, 31, xs)
    assert max(ref.mismatch(out[..., k], want[..., k]) for k in range(5)) < TOL
    key = (0, 8, f32, True)
    f = ens_inputs(key)[0]
    buf = torch.zeros(f.numel() + 3, device=dev)
    buf[3:] = f.reshape(-1).to(dev)
    fs = buf[3:].view(f.shape)
    assert fs.data_ptr() % 16 == 12 and fs.is_contiguous()
    skill, ss, hist = restatement(key)
    out = _ens(key, dev, 7, fs)
    rel, zeros = bin_errors(out[..., 2:], hist)
    assert max(ref.mismatch(out[..., 0], skill), ref.mismatch(out[..., 1], ss), rel) < TOL and zeros


def _class_cases(dev):
    """(name, module, inputs, fp64 value) of every class on the large grid, E = 9, with weights (ACC: with bias)"""
    import makani_amd as ma
    dkey, ekey = (2, f32, f32, True, True), (2, 9, f32, True)
    x, y, w, bias = det_inputs(dkey)
    f, o, we = ens_inputs(ekey)
    q = ref.quadrature_weights(GRIDS[2])
    qn = ref.quadrature_weights(GRIDS[2], normalize=True)
    out = []
    for cls, extra in [("GeometricL1", {}), ("GeometricRMSE", {}), ("GeometricACC", dict(bias=bias)),
                       ("GeometricACC", dict(bias=bias, method="micro")), ("GeometricSpread", {}), ("GeometricSSR", {}),
                       ("GeometricCRPS", {}), ("GeometricRankHistogram", {})]:
        kw = dict(channel_reduction="none", batch_reduction="sum", **extra)
        mod = getattr(ma, cls)(**_kw(2, **kw)).to(dev)
        det = cls in ("GeometricL1", "GeometricRMSE", "GeometricACC")
        a, b, wt = (x, y, w) if det else (f, o, we)
        want = ref.metric(cls, kw, a, b, qn if cls == "GeometricCRPS" else q, wt, extra.get("bias"))
        out.append((f"{cls} {extra.get('method', '')}".strip(), mod, (a.to(dev), b.to(dev), wt.to(dev)), want))
    return out


@pytest.mark.gpu
def test_classes_match_the_restatement_on_the_large_grid():
    dev = "cuda:0"
    for name, mod, args, want in _class_cases(dev):
        out = mod(*args)
        err = ref.mismatch(out, want)
        print(f"{name}: {err:.2e}")
        assert out.shape == want.shape and out.dtype == torch.float32 and not out.requires_grad and err < TOL, (name, err)


@pytest.mark.gpu
def test_recorded_reference_cases_on_the_gpu():
    """the 17 x 32 cases recorded from the reference's classes (tests/test_metrics.py pins the restatement to them) through the HIP
    classes: every variant's value (NaN where the reference has NaN: one member), and the counts under weights"""
    import makani_amd as ma
    dev = "cuda:0"
    cases = ref.load_cases(load_golden("metrics.npz"))
    assert len(cases) == 23
    for name, c in cases.items():
        a, b = c["a"].to(dev), c["b"].to(dev)
        w = c["weights"].to(dev) if c["weights"] is not None else None
        for (cr, br), rec in c["variants"].items():
            kw = dict(c["kwargs"], channel_reduction=cr, batch_reduction=br)
            if c["bias"] is not None:
                kw["bias"] = c["bias"]
            mod = getattr(ma, c["cls"])(**kw).to(dev)
            out = mod(a, b, w)
            err = ref.mismatch(out, rec["out"])
            print(f"{name} {cr}-{br}: {err:.2e}")
            assert out.shape == rec["out"].shape and err < TOL, (name, cr, br, err)
            if w is not None and rec["counts"] is not None:
                counts = mod.compute_counts(a, w)
                assert counts.shape == rec["counts"].shape and ref.mismatch(counts, rec["counts"]) < TOL, (name, cr, br)


@pytest.mark.gpu
def test_a_deterministic_and_an_ensemble_call_replay_from_a_captured_graph():
    import makani_amd as ma
    dev = "cuda:0"
    dkey, ekey = (2, f32, bf16, True, True), (2, 9, f32, True)
    x, y, w, bias = (t.to(dev) for t in det_inputs(dkey))
    f, o, we = (t.to(dev) for t in ens_inputs(ekey))
    quad = _q(2, dev)
    ssr = ma.GeometricSSR(**_kw(2, channel_reduction="none", batch_reduction="none")).to(dev)
    rh = ma.GeometricRankHistogram(**_kw(2, channel_reduction="none", batch_reduction="none")).to(dev)

    def run(x_, f_):
        return ma.deterministic_sums(x_, y, quad, bias=bias, weight=w), ssr(f_, o, we), rh(f_, o, we)

    run(x, f)                                               # loads the library outside the capture
    sx, sf = x.clone(), f.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            outs = run(sx, sf)
    torch.cuda.current_stream().wait_stream(stream)
    gen = torch.Generator().manual_seed(99)
    for _ in range(2):
        nx = x + 0.5 * torch.randn(x.shape, generator=gen).to(dev)
        nf = f + 0.5 * torch.randn(f.shape, generator=gen).to(dev)
        sx.copy_(nx)
        sf.copy_(nf)
        graph.replay()
        torch.cuda.synchronize()
        want = run(nx, nf)
        assert all(torch.equal(a, b) for a, b in zip(outs, want))


# ---- several processes on one GPU ---------------------------------------------------------------------------------------
def _worker_ensemble(rank, world, rendezvous):
    """two ensemble ranks, four members each: SSR and rank histogram with ensemble_distributed=True, Spread as it is (it follows
    the group), against the serial modules (built before the tree exists) on the gathered ensemble"""
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        img, El = (19, 36), 4
        kw = dict(grid_type="equiangular", img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_reduction="none", batch_reduction="sum")
        serial = {cls: getattr(ma, cls)(**kw).to(dev) for cls in ("GeometricSpread", "GeometricSSR", "GeometricRankHistogram")}
        assert not any(m.ensemble_distributed for m in serial.values())
        mcomm.init(1, 1, ensemble=2)
        ie = mcomm.get_rank("ensemble")
        assert mcomm.get_size("ensemble") == 2 and ie == rank
        torch.manual_seed(3)
        f_all = torch.randn(2, 2 * El, C, *img)
        o, w = torch.randn(2, C, *img), torch.rand(2, C, *img) + 0.5
        o[..., ::5] = f_all[:, 5, :, :, ::5]                # ties with a member held by the other rank, too
        o, w = o.to(dev), w.to(dev)
        for cls, ser in serial.items():
            par = getattr(ma, cls)(ensemble_distributed=True, **kw).to(dev)
            assert par.ensemble_distributed
            for wt in (None, w):
                want = ser(f_all.to(dev), o, wt)
                out = par(f_all[:, ie * El:(ie + 1) * El].to(dev), o, wt)
                err = ref.mismatch(out, want)
                print(f"rank {rank} {cls} weights {wt is not None}: {err:.2e}", flush=True)
                assert out.shape == want.shape and err < TOL, (cls, err)


def _worker_spatial(rank, world, rendezvous):
    """h2 x w2 on a 37 x 72 grid (19 + 18 latitudes): all seven classes with spatial_distributed=True on the local shard, ACC
    with a climatology (cut to the shard by the constructor), against the serial modules on the whole grid"""
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        from makani_amd import distributed as thd
        dev = "cuda:0"
        img = (37, 72)
        kw = dict(grid_type="equiangular", img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_reduction="none", batch_reduction="sum")
        torch.manual_seed(5)
        common = torch.randn(2, C, *img)
        x, y = common + torch.randn(2, C, *img), common + torch.randn(2, C, *img)
        f = common.unsqueeze(1) + torch.randn(2, 5, C, *img)
        w, bias = torch.rand(2, C, *img) + 0.5, 0.3 * torch.randn(C, *img)
        forms = [("GeometricL1", {}), ("GeometricRMSE", {}), ("GeometricACC", dict(bias=bias)), ("GeometricACC", dict(bias=bias, method="micro")),
                 ("GeometricSpread", {}), ("GeometricSSR", {}), ("GeometricCRPS", {}), ("GeometricRankHistogram", {})]
        want = []
        for cls, extra in forms:            # serial modules and values first: no tree yet, the bias stays whole
            ser = getattr(ma, cls)(**extra, **kw).to(dev)
            assert not ser.quadrature.distributed
            a = x if cls in ("GeometricL1", "GeometricRMSE", "GeometricACC") else f
            want.append(ser(a.to(dev), y.to(dev), w.to(dev)))
        _, ih, iw = mcomm.init(2, 2)
        hsz, wsz = thd.compute_split_shapes(img[0], 2), thd.compute_split_shapes(img[1], 2)
        hs = slice(sum(hsz[:ih]), sum(hsz[:ih + 1]))
        ws = slice(sum(wsz[:iw]), sum(wsz[:iw + 1]))
        assert hsz == [19, 18]
        for (cls, extra), wnt in zip(forms, want):
            par = getattr(ma, cls)(spatial_distributed=True, **extra, **kw).to(dev)
            assert par.quadrature.distributed and par.quadrature.quad_weight.shape[-2:] == (hsz[ih], wsz[iw])
            if "bias" in extra:
                assert par.bias.shape == (C, hsz[ih], wsz[iw])
            a = x if cls in ("GeometricL1", "GeometricRMSE", "GeometricACC") else f
            out = par(a[..., hs, ws].to(dev), y[..., hs, ws].to(dev), w[..., hs, ws].to(dev))
            err = ref.mismatch(out, wnt)
            print(f"rank {rank} (h {ih}, w {iw}) {cls} {extra.get('method', '')}: {err:.2e}", flush=True)
            assert out.shape == wnt.shape and err < TOL, (cls, err)


@pytest.mark.gpu
def test_ensemble_parallel_metrics_match_serial():
    launch(_worker_ensemble, 2, limit=240)


@pytest.mark.gpu
def test_spatially_parallel_metrics_match_serial():
    launch(_worker_spatial, 4, limit=240)
