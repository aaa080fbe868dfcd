"""SpectralCoherenceLoss, CoherenceRegularization and SpectralRegularization (csrc/egram.hip) without a GPU: the fp64
restatement of tests/_coherence_ref.py against fixtures recorded in double precision from the reference's own classes
(tools/make_coherence_golden.py); the conditioning of every input of tests/test_gpu_coherence.py (the reference's formula in
plain fp32 torch meets the GPU tolerance on them, with margin); the host side of the kernel's interface — slot order, weights,
triangle offset — and the constructor / error contract of the three classes."""
import math

import pytest
import torch

import _coherence_ref as ref
import test_gpu_coherence as gpu
from conftest import load_golden, rel_l2

KW = dict(img_shape=(9, 16), crop_shape=(9, 16), crop_offset=(0, 0), channel_names=["u500", "v500", "t2m"], grid_type="equiangular")
NAMES = ["coherence_default", "coherence_relative_per_channel", "coherence_single_member", "coherence_lmax", "cohreg_band_inter",
         "cohreg_default_single_member", "cohreg_default", "specreg_default", "specreg_logarithmic", "specreg_four_dimensional"]
# The fp32 formula has to meet the GPU tolerance with this factor to spare.  The HIP path evaluates the same formula in fp32
# in two stages of its own, the transform and the per-degree sums, each in another order than torch's: each may be as wrong as
# the whole torch evaluation here, which asks for a factor 2; 4 leaves as much again.
MARGIN = 4.0
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(ref.load_cases(load_golden("coherence_losses.npz")))
    return _CASES


@pytest.mark.parametrize("name", NAMES)
def test_fp64_restatement_matches_the_reference_fixtures(name):
    """value and (autograd) gradient of the test-side formulas against the reference recorded in double precision"""
    c = cases()[name]
    a = c["a"].double().requires_grad_(True)
    out = ref.reference(c["cls"], c["kwargs"], a, c["b"])
    (g,) = torch.autograd.grad(out.sum(), a)
    assert out.shape == c["out"].shape and c["out"].dtype == torch.float64
    print(f"{name}: value {rel_l2(out, c['out']):.2e} gradient {rel_l2(g, c['grad']):.2e}")
    assert rel_l2(out, c["out"]) <= 1e-12, (name, rel_l2(out, c["out"]))
    assert rel_l2(g, c["grad"]) <= 1e-12, (name, rel_l2(g, c["grad"]))


def test_the_fixture_covers_what_it_should():
    cs = cases()
    assert sorted(cs) == sorted(NAMES)
    members = {n: (c["a"].shape[1] if c["a"].dim() == 5 else 0) for n, c in cs.items()}
    assert members == {"coherence_default": 3, "coherence_relative_per_channel": 4, "coherence_single_member": 1, "coherence_lmax": 3,
                       "cohreg_band_inter": 3, "cohreg_default_single_member": 1, "cohreg_default": 3, "specreg_default": 3,
                       "specreg_logarithmic": 2, "specreg_four_dimensional": 0}
    assert cs["coherence_default"]["out"].shape == (2, 1) and cs["coherence_relative_per_channel"]["out"].shape == (2, 3)
    assert cs["coherence_lmax"]["kwargs"]["lmax"] == 12 and cs["specreg_logarithmic"]["kwargs"]["logarithmic"]
    assert cs["cohreg_band_inter"]["kwargs"] == dict(cs["cohreg_default"]["kwargs"], lmin=3, lmax=12, ensemble_coherence_weight=0.5)


# ---- the reference's formulation in plain fp32 torch ----------------------------------------------------------------------------
def _fp32_gram(f, o, q):
    """the broadcast products of the reference classes: PSDs (E, ...), observation PSD, cross spectra (E, ...), pairs (E, E, ...)"""
    f = torch.moveaxis(f, 1, 0)
    o = o.unsqueeze(0)
    psd_f = (q * f.abs().square()).sum(dim=-1)
    psd_o = (q * o.abs().square()).sum(dim=-1)
    cross = (q * (f.conj() * o).real).sum(dim=-1)
    pairs = (q * (f.unsqueeze(0).conj() * f.unsqueeze(1)).real).sum(dim=-1)
    return psd_f, psd_o, cross, pairs


def _fp32_kernel(shape, what, tri=None):
    f, o, q, dG = gpu.kernel_inputs(shape, tri)
    fr = f.clone().requires_grad_(True)
    psd_f, psd_o, cross, pairs = _fp32_gram(fr, o, q)
    E = shape[4]
    full = {(i, i): psd_f[i] for i in range(E)}
    full[(E, E)] = psd_o[0]
    full.update({(e, E): cross[e] for e in range(E)})
    full.update({(i, j): pairs[j, i] for i in range(E) for j in range(i + 1, E)})
    G = torch.stack([full[ij] for ij in ref.slots(E, what)], dim=-1)
    (g,) = torch.autograd.grad((G * dG[..., :G.shape[-1]]).sum(), fr)
    return G.detach(), g


@pytest.mark.parametrize("what", sorted(gpu.WHATS), ids=str)
@pytest.mark.parametrize("shape", gpu.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_inputs_let_the_fp32_formula_meet_the_tolerance(shape, what):
    w = gpu.WHATS[what]
    G, g = _fp32_kernel(shape, w)
    want, gw = gpu.kernel_reference(shape, w)
    errs = gpu.worst(G, want), rel_l2(G, want), gpu.worst(torch.view_as_real(g), torch.view_as_real(gw)), rel_l2(g, gw)
    print(f"{shape} {what}: fp32 torch formula vs complex128, G {errs[0]:.2e} / {errs[1]:.2e} gradient {errs[2]:.2e} / {errs[3]:.2e}")
    assert MARGIN * max(errs) < gpu.TOL, errs


def _fp32_loss(cls, kw, f, o):
    """the three reference forwards, restated in fp32 torch with the broadcast products (oracle transform in fp32)"""
    from oracle import sht as osht
    img = tuple(kw["img_shape"])
    L = ref.bandlimit(img, kw["grid_type"], kw.get("lmax"))
    sht = osht.RealSHT(*img, lmax=L, mmax=L, grid=kw["grid_type"])
    q = ref.weights(L, L, torch.float32) * (4.0 * math.pi)
    eps = kw.get("eps", 1e-10 if cls == "SpectralRegularization" else 1e-6)
    if cls == "SpectralRegularization":
        pf = (q * (sht(f.float()).abs().pow(2) / (4.0 * math.pi))).sum(dim=-1)
        po = (q * (sht(o.float().unsqueeze(1)).abs().pow(2) / (4.0 * math.pi))).sum(dim=-1)
        if kw.get("logarithmic", False):
            pf, po = torch.log(pf), torch.log(po)
        return ((pf - po).abs().sum(dim=1) / float(f.shape[1])).sum(dim=-1) / float(L)
    E = f.shape[1]
    psd_f, psd_o, cross, pairs = _fp32_gram(sht(f.float()) / math.sqrt(4.0 * math.pi), sht(o.float()) / math.sqrt(4.0 * math.pi), q)
    coh_obs = cross / torch.sqrt(psd_f * psd_o + eps)
    coh_f = pairs / torch.sqrt(psd_f.unsqueeze(0) * psd_f.unsqueeze(1) + eps)
    spread = torch.where(torch.eye(E).bool().reshape(E, E, 1, 1, 1), 0.0, 1.0 - coh_f).sum(dim=(0, 1))
    spread = spread / float(E * (E - 1)) if E > 1 else torch.zeros_like(spread)
    if cls == "CoherenceRegularization":
        loss = (1.0 - coh_obs).sum(dim=0) / float(E)
        w = kw.get("ensemble_coherence_weight", 0.0)
        if w != 0.0 and E > 1:
            loss = loss + w * spread
        lmin = kw.get("lmin") or 0
        return loss[..., lmin:].sum(dim=-1) / float(L - lmin)
    skill = (psd_f - psd_o).square()
    if kw.get("relative", False):
        skill = skill / (psd_o + eps)
    skill = skill.sum(dim=0) / float(E)
    coh = (1.0 - coh_obs).sum(dim=0) / float(E) - 0.5 * spread
    loss = skill + 2.0 * coh * (1.0 if kw.get("relative", False) else psd_o.squeeze(0))
    loss = loss.sum(dim=-1)
    return loss.sum(dim=-1, keepdim=True) if kw.get("channel_reduction", True) else loss


@pytest.mark.parametrize("form,E", gpu.LOSS_CASES, ids=lambda v: str(v))
def test_loss_inputs_let_the_fp32_formula_meet_the_tolerance(form, E):
    cls, kw = gpu.loss_kwargs(form)
    f, o, g_out = gpu.loss_inputs(form, E)
    fr = f.clone().requires_grad_(True)
    val = _fp32_loss(cls, kw, fr, o)
    (g,) = torch.autograd.grad((val * g_out).sum(), fr)
    want, gw = gpu.restatement(form, E)
    errs = gpu.worst(val, want), rel_l2(val, want), gpu.worst(g, gw), rel_l2(g, gw)
    print(f"{cls} {gpu.FORMS[form][1]} E={E}: fp32 torch formula vs fp64 restatement, value {errs[0]:.2e} / {errs[1]:.2e} "
          f"gradient {errs[2]:.2e} / {errs[3]:.2e}")
    assert MARGIN * max(errs) < gpu.TOL, errs


@pytest.mark.parametrize("name", NAMES)
def test_recorded_inputs_let_the_fp32_formula_meet_the_tolerance(name):
    c = cases()[name]
    a = c["a"].clone().requires_grad_(True)
    val = _fp32_loss(c["cls"], c["kwargs"], a if a.dim() == 5 else a.unsqueeze(1), c["b"])
    (g,) = torch.autograd.grad(val.sum(), a)
    errs = gpu.worst(val, c["out"]), rel_l2(val, c["out"]), gpu.worst(g, c["grad"]), rel_l2(g, c["grad"])
    print(f"{name}: fp32 torch formula vs the record, value {errs[0]:.2e} / {errs[1]:.2e} gradient {errs[2]:.2e} / {errs[3]:.2e}")
    assert MARGIN * max(errs) < gpu.TOL, errs


# ---- the host side of the kernel's interface ------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 3, 8, 9, 32])
def test_slot_order(E):
    from makani_amd.losses import EGRAM_DIAG, EGRAM_FULL, EGRAM_OBS, egram_slot, egram_slots
    assert (EGRAM_DIAG, EGRAM_OBS, EGRAM_FULL) == (0, 1, 2)
    n = E + 1
    assert (egram_slots(E, EGRAM_DIAG), egram_slots(E, EGRAM_OBS), egram_slots(E, EGRAM_FULL)) == (n, n + E, n + E + E * (E - 1) // 2)
    order = ref.slots(E, 2)
    assert len(order) == egram_slots(E, EGRAM_FULL) == n * (n + 1) // 2
    for k, (i, j) in enumerate(order):          # a bijection onto [0, K), symmetric, and the restatement's own formula
        assert egram_slot(i, j, E) == egram_slot(j, i, E) == ref.slot(i, j, E) == k
    assert order[:n] == [(i, i) for i in range(n)] and order[n:n + E] == [(e, E) for e in range(E)]
    pairs = order[n + E:]
    assert pairs == sorted(pairs) and all(i < j < E for i, j in pairs)
    # the pair slots are those of the energy scores (pair_index of csrc/escore.hip: E + i (2 E - i - 1) / 2 + j - i - 1), shifted by n
    assert all(egram_slot(i, j, E) - n == E + i * (2 * E - i - 1) // 2 + (j - i - 1) for i, j in pairs)
    with pytest.raises(IndexError):
        egram_slot(0, E + 1, E)


@pytest.mark.parametrize("shard", [(0, 0, 19, 19), (0, 10, 19, 9), (10, 0, 9, 10), (10, 10, 9, 9), (4, 7, 5, 3)], ids=str)
def test_weights_and_triangle_offset_of_a_shard(shard):
    from makani_amd.losses import egram_weights
    l_off, m_off, Ll, Ml = shard
    q, tri_off = egram_weights(19, 19, l_off, m_off, Ll, Ml)
    assert q.shape == (Ll, Ml) and q.dtype == torch.float32 and q.is_contiguous() and tri_off == l_off - m_off
    for l in range(Ll):
        for m in range(Ml):
            gl, gm = l + l_off, m + m_off
            want = 0.0 if gm > gl else (1.0 if gm == 0 else 2.0) / (4.0 * math.pi)
            assert float(q[l, m]) == pytest.approx(want, rel=1e-7)
            assert (float(q[l, m]) != 0.0) == (m <= l + tri_off)          # what the kernel skips is exactly where q is zero
    assert torch.equal(egram_weights(19, 19)[0], egram_weights(19, 19, 0, 0, 19, 19)[0]) and egram_weights(19, 19)[1] == 0
    assert rel_l2(q, ref.weights(19, 19)[l_off:l_off + Ll, m_off:m_off + Ml]) < 1e-7


def test_constructor_contract():
    import makani_amd as ma
    c = ma.SpectralCoherenceLoss(**KW)
    assert c.type == "probabilistic" and c.n_channels == 1 and ma.SpectralCoherenceLoss(channel_reduction=False, **KW).n_channels == 3
    assert (c.relative, c.channel_reduction, c.eps, c.ensemble_weights) == (False, True, 1.0e-6, None)
    assert not c.ensemble_distributed and not c.spatial_distributed and c.sht.lmax == 4
    assert c.compute_channel_weighting("auto", None).tolist() == [1.0]
    assert ma.SpectralCoherenceLoss(channel_reduction=False, **KW).compute_channel_weighting("auto").tolist() == pytest.approx([0.5, 0.5, 1.0])
    tri = torch.tensor([[1.0, 0, 0, 0], [1, 2, 0, 0], [1, 2, 2, 0], [1, 2, 2, 2]])
    assert torch.equal(c.lm_weights, tri)
    r = ma.CoherenceRegularization(lmin=1, lmax=3, ensemble_coherence_weight=0.25, **KW)
    assert r.type == "probabilistic" and r.n_channels == 3 and (r.lmin, r.ensemble_coherence_weight, r.eps) == (1, 0.25, 1.0e-6)
    assert r.sht.lmax == 3 and torch.equal(r.m_weights, tri[:3, :3]) and r.l_band.tolist() == [0.0, 1.0, 1.0] and float(r.band_size) == 2.0
    assert ma.CoherenceRegularization(**KW).lmin == 0 and r.ensemble_weights is None
    s = ma.SpectralRegularization(**KW)
    assert s.type == "probabilistic" and s.n_channels == 3 and (s.eps, s.logarithmic) == (1.0e-10, False)
    assert torch.equal(s.lm_weights, tri) and not s.ensemble_distributed
    assert s.compute_channel_weighting("auto").tolist() == pytest.approx([0.5, 0.5, 1.0])
    for mod in (c, r, s):
        assert len(mod.state_dict()) == 0
        assert torch.equal(mod.gram_weights, tri[:mod.sht.lmax, :mod.sht.lmax] / (4.0 * math.pi)) and mod._tri_off == 0


def test_errors_on_cpu_tensors():
    import makani_amd as ma
    f4, f5, o = torch.zeros(2, 3, 9, 16), torch.zeros(2, 2, 3, 9, 16), torch.zeros(2, 3, 9, 16)
    with pytest.raises(ValueError, match="forecasts tensor expected to have 5 dimensions but found 4"):
        ma.SpectralCoherenceLoss(**KW)(f4, o)
    with pytest.raises(ValueError, match="forecasts expected 5 dims, got 4"):
        ma.CoherenceRegularization(**KW)(f4, o)
    with pytest.raises(ValueError, match="forecasts tensor expected to have 4 or 5 dimensions but found 3"):
        ma.SpectralRegularization(**KW)(f4[0], o)
    with pytest.raises(ValueError, match=r"lmin \(4\) must be smaller than the SHT truncation lmax \(4\), otherwise the band is empty"):
        ma.CoherenceRegularization(lmin=4, **KW)
    big = torch.zeros(1, 33, 3, 9, 16)
    for cls in (ma.SpectralCoherenceLoss, ma.CoherenceRegularization, ma.SpectralRegularization):
        with pytest.raises(NotImplementedError, match="ensemble size 33"):
            cls(**KW)(big, o[:1])
        with pytest.raises(RuntimeError, match="GPU"):                  # no CPU fallback
            cls(**KW)(f5, o)
    with pytest.raises(RuntimeError, match="GPU"):
        ma.SpectralRegularization(**KW)(f4, o)
