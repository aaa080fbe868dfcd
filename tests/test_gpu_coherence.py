"""SpectralCoherenceLoss, CoherenceRegularization and SpectralRegularization on the GPU (csrc/egram.hip) against the fp64
restatement of tests/_coherence_ref.py.

Kernel level: ``EnsembleGramFn`` against the complex128 einsum, entry by entry, and its autograd with a random dG, at the
smallest shapes at which each mechanism of the kernel can fail (KERNEL_SHAPES), for the three row truncations.  Loss level: the
cases recorded from the reference's own classes (17 x 32), a second, unrecorded grid (19 x 36) with E = 1, 2, 5, 9, bf16
forecasts, the error contract, and the parallel forms (2 ensemble ranks; h2 x w2) against the serial modules.

Tolerance: 1e-5 of the largest reference magnitude (and 1e-5 relative L2, as tests/test_gpu_restloss.py), on value and gradient.
The inputs are independent random fields: identical members, or a member equal to the observation, would put 1 - coh into
cancellation; they appear in the sign / zero test only.  tests/test_coherence.py asserts without a GPU that the reference's
formula in plain fp32 torch meets the same tolerance on every input of this file.
Measured on an MI355X, worst case over the cases of a kind (largest deviation / relative L2): Gram rows 9.4e-08 / 5.3e-08, their
gradient 2.4e-07 / 1.1e-07; losses on the 19 x 36 grid, value 3.1e-07 / 2.8e-07, gradient 1.3e-06 / 6.1e-07 (the logarithmic
spectral regularisation at E = 9; the fp32 torch formula: 1.9e-06 / 8.6e-07); recorded cases, value 4.7e-07, gradient
5.7e-07; two ensemble ranks and h2 x w2 against the serial modules <= 1.3e-07."""
import pytest
import torch

import _coherence_ref as ref
from _ranks import launch, ranks
from conftest import load_golden, rel_l2

TOL = 1e-5
OFF = 1 << 30
WHATS = {"diag": 0, "obs": 1, "full": 2}
# B, C, L, M, E
KERNEL_SHAPES = [
    (2, 3, 5, 5, 1),           # n = 2; M < 64; 30 rows: not a multiple of the 4 waves of a block
    (2, 1, 7, 64, 7),          # n = 8: exactly one full tile; M = one full wave stride
    (1, 2, 6, 33, 8),          # n = 9: the second tile holds one field
    (1, 2, 9, 70, 3),          # M > 64 and not a multiple
    (1, 1, 4, 130, 16),        # n = 17: three tiles, off-diagonal tile pairs
    (1, 1, 3, 20, 32),         # n = 33: five tiles, 3 rows
]
NAMES = ["u500", "v500", "t2m"]
IMG2 = (19, 36)                # the unrecorded grid: lmax = mmax = 9
ES = [1, 2, 5, 9]
FORMS = [("SpectralCoherenceLoss", dict()), ("SpectralCoherenceLoss", dict(relative=True, channel_reduction=False)),
         ("CoherenceRegularization", dict()), ("CoherenceRegularization", dict(lmin=2, lmax=8, ensemble_coherence_weight=0.5)),
         ("SpectralRegularization", dict()), ("SpectralRegularization", dict(logarithmic=True))]
LOSS_CASES = [(form, E) for form in range(len(FORMS)) for E in ES]


def worst(a, b):
    """the largest deviation as a fraction of the largest reference magnitude"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def triangle(L, M, t):
    """1 where order m of degree l is kept under the offset t: m <= l + t"""
    return (torch.arange(M).reshape(1, -1) <= torch.arange(L).reshape(-1, 1) + t).double()


def kernel_inputs(shape, tri=None):
    """white complex coefficients, positive weights (zeroed beyond the triangle of offset ``tri``), a random dG for all slots"""
    B, C, L, M, E = shape
    gen = torch.Generator().manual_seed(1000 * E + M)
    f = torch.complex(torch.randn(B, E, C, L, M, generator=gen), torch.randn(B, E, C, L, M, generator=gen))
    o = torch.complex(torch.randn(B, C, L, M, generator=gen), torch.randn(B, C, L, M, generator=gen))
    q = torch.rand(L, M, generator=gen) + 0.5
    if tri is not None:
        q = q * triangle(L, M, tri).float()
    dG = torch.randn(B, C, L, E + 1 + E + E * (E - 1) // 2, generator=gen)
    return f, o, q, dG


_KREF = {}


def kernel_reference(shape, what, tri=None):
    """(G rows, gradient of sum(G dG) with respect to the members) in complex128 / fp64, computed once per process"""
    key = (shape, what, tri)
    if key not in _KREF:
        f, o, q, dG = kernel_inputs(shape, tri)
        fr = f.to(torch.complex128).requires_grad_(True)
        G = ref.gram_rows(fr, o, q.double(), what)
        (g,) = torch.autograd.grad((G * dG[..., :G.shape[-1]].double()).sum(), fr)
        _KREF[key] = (G.detach(), g)
    return _KREF[key]


def _gram_gpu(shape, what, tri_off, tri=None, dev="cuda:0"):
    import makani_amd as ma
    f, o, q, dG = kernel_inputs(shape, tri)
    fd = f.to(dev).requires_grad_(True)
    od = o.to(dev).requires_grad_(True)
    G = ma.EnsembleGramFn.apply(fd, od, q.to(dev), what, tri_off, [])
    (G * dG[..., :G.shape[-1]].to(dev)).sum().backward()
    return G.detach(), fd.grad, od.grad


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(WHATS), ids=str)
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_rows_and_gradient_match_complex128_entry_by_entry(shape, what):
    from makani_amd.losses import egram_slot, egram_slots
    B, C, L, M, E = shape
    w = WHATS[what]
    G, gf, go = _gram_gpu(shape, w, OFF)
    G2, gf2, _ = _gram_gpu(shape, w, OFF)
    assert torch.equal(G, G2) and torch.equal(torch.view_as_real(gf), torch.view_as_real(gf2))          # run to run: bit-identical
    assert go is None                                                                                    # the observation: no gradient
    want, gw = kernel_reference(shape, w)
    assert G.shape == want.shape == (B, C, L, egram_slots(E, w)) and G.dtype == torch.float32
    scale = float(want.abs().max())
    for k, (i, j) in enumerate(ref.slots(E, w)):          # slot order, entry by entry
        assert egram_slot(i, j, E) == k
        err = float((G[..., k].cpu().double() - want[..., k]).abs().max()) / scale
        assert err <= TOL, (shape, what, (i, j), err)
    errs = worst(G, want), rel_l2(G, want), worst(torch.view_as_real(gf), torch.view_as_real(gw)), rel_l2(gf, gw)
    print(f"{shape} {what}: G {errs[0]:.2e} / {errs[1]:.2e}  gradient {errs[2]:.2e} / {errs[3]:.2e}")
    assert gf.shape == (B, E, C, L, M) and gf.dtype == torch.complex64 and max(errs) <= TOL, errs


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, -2, 3])
@pytest.mark.parametrize("shape", [KERNEL_SHAPES[0], KERNEL_SHAPES[3], KERNEL_SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_skipping_the_structural_zeros_changes_nothing(shape, tri):
    """tri_off = tri with q zeroed beyond that triangle against "off" on the same q: the same sums and gradient; exact zeros
    (bits) at the skipped orders"""
    B, C, L, M, E = shape
    skipped = (triangle(L, M, tri) == 0).reshape(1, 1, 1, L, M, 1).expand(B, E, C, L, M, 2)
    assert int(skipped.sum()) > 0
    for what in sorted(WHATS.values()):
        G, gf, _ = _gram_gpu(shape, what, tri, tri)
        G0, gf0, _ = _gram_gpu(shape, what, OFF, tri)
        assert torch.equal(G, G0) and torch.equal(torch.view_as_real(gf), torch.view_as_real(gf0)), (shape, what, tri)
        bits = torch.view_as_real(gf).cpu().view(torch.int32)
        assert bool((bits[skipped] == 0).all())
        want, gw = kernel_reference(shape, what, tri)
        assert max(worst(G, want), worst(torch.view_as_real(gf), torch.view_as_real(gw))) <= TOL


@pytest.mark.gpu
def test_signs_and_zeros_of_degenerate_ensembles():
    """identical members, a member equal to the observation, a sign-flipped member: coherences +1 / -1 (not under the relative
    tolerance: 1 - coh cancels), spread exactly 0 for one member"""
    import makani_amd as ma
    dev = "cuda:0"
    kw = dict(img_shape=IMG2, crop_shape=IMG2, crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")
    gen = torch.Generator().manual_seed(5)
    o = (4.0 * torch.randn(2, 3, *IMG2, generator=gen)).to(dev)
    reg = ma.CoherenceRegularization(eps=0.0, lmin=1, **kw).to(dev)
    same = reg(torch.stack([o, o], dim=1), o)
    flipped = reg(torch.stack([-o, -o], dim=1), o)
    assert float(same.abs().max()) < 1e-5 and float((flipped - 2.0).abs().max()) < 1e-5
    inter = ma.CoherenceRegularization(eps=0.0, lmin=1, ensemble_coherence_weight=1.0, **kw).to(dev)
    assert float((inter(torch.stack([o, -o], dim=1), o) - 3.0).abs().max()) < 1e-5          # mean(0, 2) + 1 * (1 - (-1))
    coh = ma.SpectralCoherenceLoss(channel_reduction=False, **kw).to(dev)
    one = torch.randn(2, 1, 3, *IMG2, generator=gen).to(dev)
    want = ref.reference("SpectralCoherenceLoss", dict(kw, channel_reduction=False), one.cpu(), o.cpu())
    assert worst(coh(one, o), want) <= TOL                                                  # E = 1: no spread term at all


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(WHATS), ids=str)
def test_forward_and_backward_replay_from_a_captured_graph(what):
    import makani_amd as ma
    dev, shape, w = "cuda:0", KERNEL_SHAPES[3], WHATS[what]
    f, o, q, dG = kernel_inputs(shape)
    K = len(ref.slots(shape[4], w))
    f, o, q, dG = f.to(dev), o.to(dev), q.to(dev), dG[..., :K].contiguous().to(dev)

    def run(x):
        x = x.clone().requires_grad_(True)
        G = ma.EnsembleGramFn.apply(x, o, q, w, 0, [])
        return G, torch.autograd.grad((G * dG).sum(), x)[0]

    run(f)
    static = f.clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            G = ma.EnsembleGramFn.apply(static, o, q, w, 0, [])
            (g,) = torch.autograd.grad((G * dG).sum(), static)
    torch.cuda.current_stream().wait_stream(stream)
    gen = torch.Generator().manual_seed(99)
    for _ in range(2):
        fresh = f + 0.5 * torch.view_as_complex(torch.randn(*f.shape, 2, generator=gen)).to(dev)
        with torch.no_grad():
            static.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        Gw, gw = run(fresh)
        assert torch.equal(G, Gw) and torch.equal(torch.view_as_real(g), torch.view_as_real(gw))


# ---- the losses ---------------------------------------------------------------------------------------------------------------
def loss_kwargs(form, img=IMG2):
    cls, extra = FORMS[form]
    return cls, dict(img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular", **extra)


def loss_inputs(form, E, img=IMG2, dtype=torch.float32):
    """independent white fields with distinct means (the mean is the ONE coefficient of degree 0: without it that degree's
    power is a small random number, and the relative form divides by it): members, observation, the gradient of the output"""
    cls, kw = loss_kwargs(form, img)
    gen = torch.Generator().manual_seed(100 * form + E)
    f = (2.0 * torch.randn(2, E, len(NAMES), *img, generator=gen) + 0.5 + 0.125 * torch.arange(E).reshape(1, E, 1, 1, 1)).to(dtype)
    o = 2.0 * torch.randn(2, len(NAMES), *img, generator=gen) + 1.0
    cout = 1 if (cls == "SpectralCoherenceLoss" and kw.get("channel_reduction", True)) else len(NAMES)
    return f, o, torch.randn(2, cout, generator=gen)


_LREF = {}


def restatement(form, E, dtype=torch.float32):
    key = (form, E, dtype)
    if key not in _LREF:
        cls, kw = loss_kwargs(form)
        f, o, g_out = loss_inputs(form, E, dtype=dtype)
        fr = f.double().requires_grad_(True)
        val = ref.reference(cls, kw, fr, o)
        (g,) = torch.autograd.grad((val * g_out.double()).sum(), fr)
        _LREF[key] = (val.detach(), g)
    return _LREF[key]


def _loss_gpu(form, E, dtype=torch.float32, dev="cuda:0"):
    import makani_amd as ma
    cls, kw = loss_kwargs(form)
    mod = getattr(ma, cls)(**kw).to(dev)
    f, o, g_out = loss_inputs(form, E, dtype=dtype)
    fd = f.to(dev).requires_grad_(True)
    out = mod(fd, o.to(dev))
    (out.float() * g_out.to(dev)).sum().backward()
    return out.detach(), fd.grad


@pytest.mark.gpu
@pytest.mark.parametrize("form,E", LOSS_CASES, ids=lambda v: str(v))
def test_losses_match_fp64_restatement_on_an_unrecorded_grid(form, E):
    out, g = _loss_gpu(form, E)
    out2, g2 = _loss_gpu(form, E)
    assert torch.equal(out, out2) and torch.equal(g, g2)
    want, gw = restatement(form, E)
    errs = worst(out, want), rel_l2(out, want), worst(g, gw), rel_l2(g, gw)
    print(f"{FORMS[form]} E={E}: value {errs[0]:.2e} / {errs[1]:.2e}  gradient {errs[2]:.2e} / {errs[3]:.2e}")
    assert out.shape == want.shape and out.dtype == torch.float32 and max(errs) <= TOL, errs


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 3, 5], ids=str)
def test_bf16_forecasts(form):
    """cast to fp32 before the transform, as the reference's ``.float()``: the value against the restatement on the
    bf16-rounded members; the gradient is the fp32 gradient rounded once to bf16 (relative error per element <= 2^-9)"""
    out, g = _loss_gpu(form, 5, torch.bfloat16)
    want, gw = restatement(form, 5, torch.bfloat16)
    errs = worst(out, want), rel_l2(out, want), rel_l2(g.float(), gw)
    print(f"{FORMS[form]} bf16: value {errs[0]:.2e} / {errs[1]:.2e}  gradient {errs[2]:.2e}")
    assert g.dtype == torch.bfloat16 and max(errs[:2]) <= TOL and errs[2] < 2.0 ** -9, errs


@pytest.mark.gpu
def test_recorded_reference_cases_on_the_gpu():
    """the 17 x 32 cases recorded from the reference's classes (tests/test_coherence.py pins the restatement to them)"""
    import makani_amd as ma
    dev = "cuda:0"
    cases = ref.load_cases(load_golden("coherence_losses.npz"))
    assert len(cases) == 10
    for name, c in cases.items():
        mod = getattr(ma, c["cls"])(**c["kwargs"]).to(dev)
        a = c["a"].to(dev).requires_grad_(True)
        out = mod(a, c["b"].to(dev))
        (g,) = torch.autograd.grad(out.sum(), a)
        errs = worst(out, c["out"]), rel_l2(out, c["out"]), worst(g, c["grad"]), rel_l2(g, c["grad"])
        print(f"{name}: value {errs[0]:.2e} / {errs[1]:.2e}  gradient {errs[2]:.2e} / {errs[3]:.2e}")
        assert out.shape == c["out"].shape and max(errs) <= TOL, (name, errs)


@pytest.mark.gpu
def test_error_contract_on_the_gpu():
    import makani_amd as ma
    dev = "cuda:0"
    kw = loss_kwargs(0)[1]
    f4, o = torch.zeros(2, 3, *IMG2, device=dev), torch.zeros(2, 3, *IMG2, device=dev)
    with pytest.raises(ValueError, match="forecasts tensor expected to have 5 dimensions but found 4"):
        ma.SpectralCoherenceLoss(**kw).to(dev)(f4, o)
    with pytest.raises(ValueError, match="forecasts expected 5 dims, got 4"):
        ma.CoherenceRegularization(**kw).to(dev)(f4, o)
    with pytest.raises(ValueError, match="forecasts tensor expected to have 4 or 5 dimensions but found 3"):
        ma.SpectralRegularization(**kw).to(dev)(f4[0], o)
    with pytest.raises(ValueError, match=r"lmin \(9\) must be smaller than the SHT truncation lmax \(9\), otherwise the band is empty"):
        ma.CoherenceRegularization(lmin=9, **kw)
    big = torch.zeros(1, 33, 3, *IMG2, device=dev)
    for cls in (ma.SpectralCoherenceLoss, ma.CoherenceRegularization, ma.SpectralRegularization):
        with pytest.raises(NotImplementedError, match="ensemble size 33"):
            cls(**kw).to(dev)(big, o[:1])
        with pytest.raises(RuntimeError, match="GPU"):
            cls(**kw)(torch.zeros(2, 2, 3, *IMG2), o.cpu())
    z = torch.zeros(1, 33, 1, 3, 4, dtype=torch.complex64, device=dev)
    with pytest.raises(NotImplementedError, match="ensemble size 33"):
        ma.EnsembleGramFn.apply(z, z[:, 0], torch.ones(3, 4, device=dev), 0, OFF, [])


# ---- several processes on one GPU ---------------------------------------------------------------------------------------------
PARALLEL_FORMS = [("SpectralCoherenceLoss", dict(channel_reduction=False)), ("SpectralCoherenceLoss", dict(relative=True)),
                  ("CoherenceRegularization", dict()), ("CoherenceRegularization", dict(lmin=2, ensemble_coherence_weight=0.5)),
                  ("SpectralRegularization", dict()), ("SpectralRegularization", dict(logarithmic=True))]


def _worker_ensemble(rank, world, rendezvous):
    """two ensemble ranks, two members each: ensemble_distributed=True against the serial modules on the gathered ensemble
    (value) and its local members (gradient)"""
    with ranks(rank, world, rendezvous, timeout=120):
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        mcomm.init(1, 1, ensemble=2)
        ie = mcomm.get_rank("ensemble")
        assert mcomm.get_size("ensemble") == 2 and ie == rank
        torch.manual_seed(3)
        El = 2
        f_all = 2.0 * torch.randn(2, 2 * El, 3, *IMG2)
        o = (2.0 * torch.randn(2, 3, *IMG2)).to(dev)
        kw = loss_kwargs(0)[1]
        for cls, extra in PARALLEL_FORMS:
            ser, par = getattr(ma, cls)(**extra, **kw).to(dev), getattr(ma, cls)(ensemble_distributed=True, **extra, **kw).to(dev)
            assert par.ensemble_distributed and not ser.ensemble_distributed
            g = torch.randn(2, ser.n_channels, generator=torch.Generator().manual_seed(11)).to(dev)
            fs = f_all.to(dev).requires_grad_(True)
            want = ser(fs, o)
            (want * g).sum().backward()
            fl = f_all[:, ie * El:(ie + 1) * El].to(dev).requires_grad_(True)
            out = par(fl, o)
            (out * g).sum().backward()
            errs = rel_l2(out, want), rel_l2(fl.grad, fs.grad[:, ie * El:(ie + 1) * El])
            print(f"rank {rank} {cls} {extra}: value {errs[0]:.2e} gradient {errs[1]:.2e}", flush=True)
            assert max(errs) < TOL, (cls, errs)


def _worker_spatial(rank, world, rendezvous):
    """h2 x w2 on a 37 x 72 grid (19 + 18 latitudes; the w rank 1 holds no order 0): spatial_distributed=True against the
    serial modules: value, and the local shard of the forecast gradient"""
    with ranks(rank, world, rendezvous, timeout=120):
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = "cuda:0"
        _, ih, iw = mcomm.init(2, 2)
        img = (37, 72)
        kw = loss_kwargs(0, img)[1]
        torch.manual_seed(5)
        f = (2.0 * torch.randn(2, 3, 3, *img)).to(dev)
        o = (2.0 * torch.randn(2, 3, *img)).to(dev)
        for cls, extra in PARALLEL_FORMS:
            ser, par = getattr(ma, cls)(**extra, **kw).to(dev), getattr(ma, cls)(spatial_distributed=True, **extra, **kw).to(dev)
            assert par.spatial_distributed and not ser.spatial_distributed
            sht = par.sht
            assert (sht.m_off != 0) == (iw == 1) and sum(sht.lat_shapes) == 37
            h0, w0 = sum(sht.lat_shapes[:ih]), sum(sht.lon_shapes[:iw])
            hs, ws = slice(h0, h0 + sht.lat_shapes[ih]), slice(w0, w0 + sht.lon_shapes[iw])
            g = torch.randn(2, ser.n_channels, generator=torch.Generator().manual_seed(11)).to(dev)
            fs = f.clone().requires_grad_(True)
            want = ser(fs, o)
            (want * g).sum().backward()
            fl = f[..., hs, ws].clone().requires_grad_(True)
            out = par(fl, o[..., hs, ws].contiguous())
            (out * g).sum().backward()
            errs = rel_l2(out, want), rel_l2(fl.grad, fs.grad[..., hs, ws])
            print(f"rank {rank} (h {ih}, w {iw}) {cls} {extra}: value {errs[0]:.2e} gradient {errs[1]:.2e}", flush=True)
            assert max(errs) < TOL, (cls, errs)


@pytest.mark.gpu
def test_ensemble_parallel_losses_match_serial():
    launch(_worker_ensemble, 2, limit=240)


@pytest.mark.gpu
def test_spatially_parallel_losses_match_serial():
    launch(_worker_spatial, 4, limit=240)
