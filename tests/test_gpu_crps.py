"""The CRPS kernels (csrc/crps.hip) against the fp64 restatement of tests/_crps_ref.py, value and forecast gradient, at the
smallest shapes that reach every path of the file:

  a  CPU: the restatement reproduces every E >= 2 case of tests/golden/crps_loss.npz (the reference's own outputs, fp32) to 1e-6
  c  type x capacity, fp32: all five types x E = 2, 3, 4, 5, 8, 9, 16, 17, 31, 32 (both sides of every capacity boundary
     EM = 2, 4, 8, 16, 32); B = 2, C = 3 (a b / c or member-stride mix-up shows); plane 91 x 180 = 16 380 points = 16 chunks,
     not a multiple of the 256-thread block, so partial[plane * gridDim.x + chunk] is summed over several chunks
  d  the capped grid: 182 x 361 = 65 702 points: mk_crps_chunks stops at 64 and some threads take a fifth stride of the
     grid-stride loop (what every 721 x 1440 training step runs, at 1/16 of the points); every type at E = 5, skillspread and
     cdf also at E = 32
  e  the tiny plane: 5 x 8 = 40 points, less than one wave; every type at E = 3
  f  dtype pairs (forecast, observation) = (bf16, f32), (bf16, bf16), (f32, bf16): every type at E = 5 and 32 on 37 x 72
     (2 664 points, 3 chunks); the bf16 gradient store and the bf16 observation load
  g  the wrapper: CRPSLoss with non-contiguous forecasts, a sliced observation view, broadcast spatial weights of shape
     (1, C, 1, 1) and (B, 1, H, W), fp64 inputs (gradient comes back fp64)
  h  more than 65 535 planes raise the library's error before any launch
  i  the complex kernel: E = 2, 3, 5, 8, 9, 17, 32 on (B, C, L, M) = (2, 3, 33, 40), spatial weights on every other case, and
     E = 3 on the 65 702-point plane; coincident members, members on the observation, NaN real / imaginary parts
The CPU check of mk_crps_chunks for these planes (1, 16, 64 chunks) is tests/test_host_logic.py::test_crps_chunk_counts.

Inputs, as tests/test_gpu_escore.py: a common field (std 10) + a member part (std 2) + 0.25 e; q a random positive vector of
sum 1 that is NOT constant along a row (an index slip along longitude shows); w uniform in [0.5, 1.5); alpha = 0.95 for the
two skillspread forms; member weights in [0.5, 1.5) for cdf at odd E; about 1 % NaN observations for the three masking types.
The member spread stays far above eps, so "gauss" never clamps (its zero-spread subgradient: tests/test_crps.py).

Tolerances.  fp32 forecasts: rel-L2 < 1e-5 on value and gradient.  bf16 forecasts: value 1e-5 (the kernel
computes in fp32 from the same rounded inputs as the restatement), gradient 2^-8 (every stored element is within half a bf16
ulp, 2^-9 relative, of the fp32 gradient; the factor 2 covers the fp32 error and the rounding mode).  A second pass on the
same inputs is bit-identical.

The kink.  A member that equals its observation sits on a kink of |f - o| whose one-sided derivative is a convention, not a
kernel property (the rank forms take 0 there, the cdf loop one side).  After rounding to bf16 (f) hundreds of members do
(about 650 of 80 000 at E = 5, 1 400 of 511 000 at E = 32); they are moved one or two bf16 steps away (f (1 + 2^-7), which
never rounds back), the test asserts that none is left and that the E = 32 bf16 forecasts do hold member-member ties (about
32 000 adjacent equal pairs in 16 000 points: the stable tie order at scale).  In fp32 the same happens about once in a
million members (o + a member part below half an ulp of o): one member of the cdf E = 17 case of (c); the fp32 inputs get
the same treatment.  Members excluded after that: 0 in every case.  Nothing else is excluded.

Measured.  The per-point code of csrc/crps.hip (crps_point, compiled for the host from the same source text, fp32, with the
plane sum, the bf16 load and the bf16 rounding of the stored gradient done in torch) against the restatement, maxima over the
group, value / gradient:  c 1.5e-7 / 8.9e-7 (cdf at E = 31);  d 1.2e-7 / 1.4e-7;  e 1.2e-7 / 1.3e-7;  f 1.2e-7 / 1.67e-3 with
bf16 forecasts (bound 2^-8 = 3.9e-3), 1.2e-7 / 1.5e-7 with fp32 forecasts.  Before the first member became the pivot of the "gauss" moments that code gave 4.9e-5 on the
gradient of gauss at E = 2 in (c) (two members 1e-3 apart around 10: the rounding of their mean is 1e-3 of the deviation);
7.2e-8 after.  The figures of the kernels themselves on the MI355X (groups c to i: grid indexing, chunk sums, the bf16
store, the wrapper and the complex kernel are reached there only) are printed by every case and have not been recorded here."""
import json

import pytest
import torch

import _crps_ref as ref
import _escore_ref
from conftest import load_golden, rel_l2

TYPES = ["skillspread", "probability weighted moment", "naive skillspread", "gauss", "cdf"]
EPS = 1.0e-6
BF16_GRAD = 2.0 ** -8


# --------------------------------------------------------------------------- #
# a. CPU: the restatement against the reference's own outputs
# --------------------------------------------------------------------------- #
def _golden_cases():
    g = load_golden("crps_loss.npz")
    return g, [(i, c) for i, c in enumerate(json.loads(str(g["cases"]))) if c["E"] >= 2]


def test_restatement_covers_every_golden_case():
    assert len(_golden_cases()[1]) == 10


@pytest.mark.parametrize("k", range(10))
def test_restatement_reproduces_golden(k):
    import makani_amd as ma
    g, cases = _golden_cases()
    i, c = cases[k]
    img = tuple(c["img"])
    if c["grid"] == "equiangular":
        q = _escore_ref.quadrature_weights(img)
    else:
        q = ma.CRPSLoss(img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_names=["a"], grid_type=c["grid"]).quad_weight_split
    f = torch.from_numpy(g[f"{i}_f"]).double().requires_grad_(True)
    o = torch.from_numpy(g[f"{i}_o"])
    w = torch.from_numpy(g[f"{i}_wgt"]) if f"{i}_wgt" in g.files else None
    ens_w = torch.from_numpy(g[f"{i}_ens_w"]) if f"{i}_ens_w" in g.files else None
    out = ref.crps(f, o, q, w, c["crps_type"], c["alpha"], EPS, ens_w)
    (df,) = torch.autograd.grad((out * torch.from_numpy(g[f"{i}_g"]).double()).sum(), f)
    ev, eg = rel_l2(out, torch.from_numpy(g[f"{i}_out"])), rel_l2(df, torch.from_numpy(g[f"{i}_df"]))
    print(f"golden {i} {c['crps_type']} E={c['E']}: value {ev:.2e} gradient {eg:.2e}")
    assert ev < 1e-6, ev
    assert eg < 1e-6, eg


# --------------------------------------------------------------------------- #
# the real kernels
# --------------------------------------------------------------------------- #
def _off_the_kink(f, o):
    """a member that equals its observation sits on the kink of |f - o|, where the one-sided derivative is a convention and
    not a property of the kernel: such members are moved off it (in f's dtype: f (1 + 2^-7) never rounds back) and none is
    left.  It happens in fp32 too: o + (a member part below half an ulp of o) rounds to o about once in a million members."""
    f = torch.where(f == o.unsqueeze(1), f * (1.0 + 2.0 ** -7), f)
    assert int((f == o.unsqueeze(1)).sum()) == 0
    return f


def _inputs(ctype, B, E, C, plane, gen, dev="cuda:0"):
    """(f, o, q, w, g_out, alpha, ens_w) on the device, fp32"""
    o = 10.0 * torch.randn(B, C, *plane, generator=gen)
    f = o.unsqueeze(1) + 2.0 * torch.randn(B, E, C, *plane, generator=gen) + 0.25 * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
    q = torch.rand(plane[0] * plane[1], generator=gen) + 0.05
    q = q / q.sum()
    w = torch.rand(B, C, *plane, generator=gen) + 0.5
    g_out = torch.randn(B, C, generator=gen)
    nan = torch.rand(B, C, *plane, generator=gen) < 0.01
    ens_w = torch.rand(E, generator=gen) + 0.5
    if ctype in ref.MASKING:
        o = torch.where(nan, torch.full_like(o, float("nan")), o)
    alpha = 0.95 if ctype in ("skillspread", "naive skillspread") else 1.0
    ens_w = ens_w.to(dev) if ctype == "cdf" and E % 2 == 1 else None
    f = _off_the_kink(f, o)
    return f.to(dev), o.to(dev), q.to(dev), w.to(dev), g_out.to(dev), alpha, ens_w


def _compare(label, ctype, f, o, q, w, g_out, alpha, ens_w, tol_v=1e-5, tol_g=1e-5):
    from makani_amd.losses import _CRPS_TYPES, CrpsFn
    runs = []
    for _ in range(2):
        fx = f.clone().requires_grad_(True)
        out = CrpsFn.apply(fx, o, q, w, _CRPS_TYPES[ctype], alpha, EPS, ens_w)
        (g,) = torch.autograd.grad((out * g_out).sum(), fx)
        runs.append((out, g))
    out, g = runs[0]
    assert g.dtype == f.dtype and g.shape == f.shape
    fr = f.double().requires_grad_(True)
    want = ref.crps(fr, o, q, w, ctype, alpha, EPS, ens_w)
    (gw,) = torch.autograd.grad((want * g_out.double()).sum(), fr)
    ev, eg = rel_l2(out, want), rel_l2(g, gw)
    print(f"{label} {ctype} E={f.shape[1]} {str(f.dtype)[6:]}/{str(o.dtype)[6:]}: value {ev:.2e} gradient {eg:.2e}")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert ev < tol_v, ev
    assert eg < tol_g, eg


@pytest.mark.gpu
@pytest.mark.parametrize("E", [2, 3, 4, 5, 8, 9, 16, 17, 31, 32])
@pytest.mark.parametrize("t", range(5))
def test_crps_type_capacity_matrix(t, E):
    gen = torch.Generator().manual_seed(1000 * t + E)
    _compare("c 91x180", TYPES[t], *_inputs(TYPES[t], 2, E, 3, (91, 180), gen))


@pytest.mark.gpu
@pytest.mark.parametrize("t,E", [(t, 5) for t in range(5)] + [(0, 32), (4, 32)])
def test_crps_capped_grid(t, E):
    gen = torch.Generator().manual_seed(2000 + 100 * t + E)
    _compare("d 182x361", TYPES[t], *_inputs(TYPES[t], 1, E, 2, (182, 361), gen))


@pytest.mark.gpu
@pytest.mark.parametrize("t", range(5))
def test_crps_tiny_plane(t):
    gen = torch.Generator().manual_seed(3000 + t)
    _compare("e 5x8", TYPES[t], *_inputs(TYPES[t], 2, 3, 3, (5, 8), gen))


@pytest.mark.gpu
@pytest.mark.parametrize("E", [5, 32])
@pytest.mark.parametrize("t", range(5))
@pytest.mark.parametrize("pair", ["bf16-f32", "bf16-bf16", "f32-bf16"])
def test_crps_dtype_pairs(pair, t, E):
    df, do = ({"bf16": torch.bfloat16, "f32": torch.float32}[s] for s in pair.split("-"))
    gen = torch.Generator().manual_seed(4000 + 100 * t + E)
    f, o, *rest = _inputs(TYPES[t], 2, E, 3, (37, 72), gen)
    f, o = f.to(df), o.to(do)
    f = _off_the_kink(f, o)                                               # in bf16: one or two steps away, never back
    assert f.dtype == df and int((f == o.unsqueeze(1)).sum()) == 0
    fs = torch.sort(f.float(), dim=1).values
    ties = int((fs[:, 1:] == fs[:, :-1]).sum())
    print(f"f {pair} {TYPES[t]} E={E}: member-member ties {ties}, members on their observation 0")
    if df == torch.bfloat16 and E == 32:
        assert ties > 0
    _compare(f"f 37x72", TYPES[t], f, o, *rest, tol_g=BF16_GRAD if df == torch.bfloat16 else 1e-5)


WRAPPER = [("non-contiguous forecasts", "skillspread"), ("observation view", "cdf"), ("weights (1, C, 1, 1)", "gauss"),
           ("weights (B, 1, H, W)", "naive skillspread"), ("fp64 inputs", "probability weighted moment")]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(WRAPPER)))
def test_crps_wrapper_paths(k):
    import makani_amd as ma
    what, ctype = WRAPPER[k]
    img, B, E, C, dev = (37, 72), 2, 5, 3, "cuda:0"
    alpha = 0.95 if "skillspread" in ctype else 1.0
    mod = ma.CRPSLoss(img_shape=img, crop_shape=img, crop_offset=(0, 0), channel_names=["a", "b", "c"], grid_type="equiangular",
                      crps_type=ctype, alpha=alpha, eps=EPS).to(dev)
    gen = torch.Generator().manual_seed(5000 + k)
    dt = torch.float64 if what == "fp64 inputs" else torch.float32
    o = 10.0 * torch.randn(B, C, *img, generator=gen, dtype=dt)
    f = o.unsqueeze(1) + 2.0 * torch.randn(B, E, C, *img, generator=gen, dtype=dt) + 0.25 * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
    assert int((f.float() == o.float().unsqueeze(1)).sum()) == 0             # no member on the kink, as the kernel sees them
    f, o = f.to(dev), o.to(dev)
    g_out = torch.randn(B, C, generator=gen).to(dev)
    w = None
    leaf = f.clone().requires_grad_(True)
    fx = leaf
    if what == "non-contiguous forecasts":
        leaf = f.transpose(0, 1).contiguous().requires_grad_(True)            # (E, B, C, H, W)
        fx = leaf.transpose(0, 1)
        assert not fx.is_contiguous()
    elif what == "observation view":
        big = torch.zeros(B, C + 2, img[0], img[1] + 3, device=dev)
        big[:, 1:C + 1, :, :img[1]] = o
        o = big[:, 1:C + 1, :, :img[1]]
        assert not o.is_contiguous()
    elif what == "weights (1, C, 1, 1)":
        w = (torch.rand(1, C, 1, 1, generator=gen) + 0.5).to(dev)
    elif what == "weights (B, 1, H, W)":
        w = (torch.rand(B, 1, *img, generator=gen) + 0.5).to(dev)
    out = mod(fx, o, w)
    (g,) = torch.autograd.grad((out * g_out).sum(), leaf)
    fr = f.double().requires_grad_(True)
    want = ref.crps(fr, o, _escore_ref.quadrature_weights(img), w, ctype, alpha, EPS)
    (gw,) = torch.autograd.grad((want * g_out.double()).sum(), fr)
    if what == "non-contiguous forecasts":
        gw = gw.transpose(0, 1)
    ev, eg = rel_l2(out, want), rel_l2(g, gw)
    print(f"g {what} {ctype}: value {ev:.2e} gradient {eg:.2e}")
    assert g.dtype == dt and g.shape == leaf.shape and out.shape == (B, C)
    assert ev < 1e-5, ev
    assert eg < 1e-5, eg


@pytest.mark.gpu
def test_crps_plane_limit_raises():
    """B * C > 65 535 planes do not fit the grid's second dimension: the library's error, before any launch"""
    from makani_amd.losses import CrpsComplexFn, CrpsFn
    dev = "cuda:0"
    f, o, q = torch.zeros(1, 2, 65536, 1, 1, device=dev), torch.zeros(1, 65536, 1, 1, device=dev), torch.ones(1, device=dev)
    with pytest.raises(RuntimeError, match="plane limit of 65535"):
        CrpsFn.apply(f, o, q, None, 0, 1.0, EPS, None)
    with pytest.raises(RuntimeError, match="plane limit of 65535"):
        CrpsComplexFn.apply(f.to(torch.complex64), o.to(torch.complex64), q, None, 1.0)
    ok = CrpsFn.apply(f[:, :, :65535], o[:, :65535], q, None, 0, 1.0, EPS, None)         # the limit itself runs
    assert ok.shape == (1, 65535) and float(ok.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("E,shape", [(E, (2, 3, 33, 40)) for E in (2, 3, 5, 8, 9, 17, 32)] + [(3, (1, 2, 182, 361))])
def test_crps_complex_kernel(E, shape):
    from makani_amd.losses import CrpsComplexFn
    B, C, L, M = shape
    dev, alpha = "cuda:0", 0.95
    gen = torch.Generator().manual_seed(6000 + E + L)

    def cn(*s):
        return torch.complex(torch.randn(*s, generator=gen), torch.randn(*s, generator=gen))
    o = 10.0 * cn(B, C, L, M)
    f = o.unsqueeze(1) + 2.0 * cn(B, E, C, L, M) + 0.25 * torch.arange(1, E + 1).reshape(1, E, 1, 1, 1)
    on_obs, tie, nan_re, nan_im = (torch.rand(B, C, L, M, generator=gen) < p for p in (0.01, 0.01, 0.005, 0.005))
    f[:, 0] = torch.where(on_obs, o, f[:, 0])                    # a member on the observation ...
    f[:, 1] = torch.where(tie, f[:, 0], f[:, 1])                 # ... two coincident members (on some points all three coincide)
    nan = torch.full_like(o.real, float("nan"))
    o = torch.complex(torch.where(nan_re, nan, o.real), torch.where(nan_im, nan, o.imag))
    q = torch.rand(L * M, generator=gen) + 0.05
    q = (q / q.sum()).to(dev)
    w = (torch.rand(B, C, L, M, generator=gen) + 0.5).to(dev) if E in (3, 8, 17) else None
    g_out = torch.randn(B, C, generator=gen).to(dev)
    f, o = f.to(dev), o.to(dev)
    assert int(on_obs.sum()) > 0 and int(tie.sum()) > 0 and int((nan_re | nan_im).sum()) > 0
    runs = []
    for _ in range(2):
        fx = f.clone().requires_grad_(True)
        out = CrpsComplexFn.apply(fx, o, q, w, alpha)
        (g,) = torch.autograd.grad((out * g_out).sum(), fx)
        runs.append((out, g))
    out, g = runs[0]
    fr = f.to(torch.complex128).requires_grad_(True)
    want = ref.crps(fr, o, q, w, "naive skillspread", alpha)
    (gw,) = torch.autograd.grad((want * g_out.double()).sum(), fr)
    ev, eg = rel_l2(out, want), rel_l2(g, gw)
    print(f"i complex {L}x{M} E={E} w={w is not None}: value {ev:.2e} gradient {eg:.2e}")
    assert g.dtype == torch.complex64 and g.shape == f.shape
    assert torch.equal(torch.view_as_real(runs[0][1]), torch.view_as_real(runs[1][1])) and torch.equal(runs[0][0], runs[1][0])
    assert ev < 1e-5, ev
    assert eg < 1e-5, eg
