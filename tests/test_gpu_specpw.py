"""The four kernels of csrc/spectral_pointwise.hip (sep_mul, sep_wgrad, diag<CONJ>, diag_wgrad) through ops.DiagContractFn /
ops.SepContractFn against the complex128 restatement tests/_specpw_ref.py, at the edges of their own tiling: a second and a
ragged K stage, several output blocks, layout padding in a block of its own, group slices off the 4-channel grid, every tile of
the weight gradient, the grid-stride branch of the streaming kernels, and tri_off != 0 (a rank's window of an h x w split).
Outputs and gradients are read back UNMASKED (s_to_complex with l_off = M), so what the kernels leave at dead positions is
compared too: the restatement holds exact zeros there.

Gate: 2e-6 relative L2 (the fp32 gate of tests/test_gpu_kernels.py, ENGINE_TOL["fp32"]); the same einsums in complex64 on the
CPU sit at 0.5 ... 1.7e-7 from complex128 at these shapes.

Worst measured on an MI355X over all cases below (each test prints its figures: pytest -s):
  diag fwd 1.6e-7, diag dgrad 1.2e-7, diag wgrad 4.7e-8, sep mul 3.9e-8, sep conj-mul 3.3e-8, sep wgrad 1.3e-7
  SpectralConv module cases (gates 1e-5 / 2e-5): y <= 2.6e-7, gx <= 2.5e-7, gw <= 2.5e-7
Not reached: the grid-stride branch of sep_wgrad_kernel with Mw = 1 (more than 4096 * 256 items of L * C / 4 would need a tensor
64 x larger than the largest here); the same loop is taken with Mw = M in the 1022-channel case."""
import ctypes as C

import pytest
import torch

import _specpw_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2e-6
TOL_OP = 1e-5                     # the gate of tests/test_gpu_model.py::test_spectral_conv_matches_reference_golden


def _randc(gen, *shape):
    return torch.randn(*shape, dtype=torch.complex64, generator=gen)


def _dead(L, M, tri_off):
    return ~R.live(L, M, tri_off, 0)


def _report(family, got, ref):
    e = rel_l2(got, ref)
    print(f"specpw {family} {e:.2e}", flush=True)
    return e


# --------------------------------------------------------------------------- #
# runners: S-layout in, S-layout out, exactly the calls SpectralConv._contract makes
# --------------------------------------------------------------------------- #
def _dirty(*tensors):
    """leave NaN-filled blocks of these tensors' sizes in torch's allocator cache: the functions under test take their outputs
    from torch.empty, which then hands those blocks out, so whatever a kernel fails to write reads back as NaN, not as the
    zeros a fresh allocation may hold"""
    blocks = [torch.full((t.numel() * (2 if t.is_complex() else 1),), float("nan"), dtype=torch.float32, device=DEV) for t in tensors]
    torch.cuda.synchronize()
    del blocks


def _diag_raw(S, w, gT, B, tri_off):
    """-> T, gS (S-layout) and gw (parameter layout) of ops.DiagContractFn"""
    from makani_amd import ops
    S = S.clone().requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    _dirty(gT, S, wd)
    T = ops.DiagContractFn.apply(S, wd, B, tri_off)
    T.backward(gT)
    return T.detach(), S.grad, wd.grad


def _sep_raw(S, w3, gT, B, tri_off):
    """w3 (C, L, Mw) complex64 -> y, gS (S-layout) and gw (C, L, Mw) of ops.SepContractFn behind ops.WeightToSFn"""
    from makani_amd import ops
    S = S.clone().requires_grad_(True)
    wd = w3.to(DEV).requires_grad_(True)
    _dirty(S, S, wd)
    y = ops.SepContractFn.apply(S, ops.WeightToSFn.apply(wd), B, tri_off)
    y.backward(gT)
    return y.detach(), S.grad, wd.grad


def _unmasked(S, B, Cc):
    from makani_amd import ops
    return ops.s_to_complex(S.contiguous(), B, Cc, l_off=S.shape[1], m_off=0)


def _pad_is_zero(S, B, Cc):
    L, M, _, R_ = S.shape
    pad = S.view(L, M, 2, B, R_ // B)[..., Cc:]
    return bool((pad == 0).all())


def _check_diag(x, w, gy, tri_off, ref):
    """x (B, Cin, L, M), w (G, Cin/G, Cout/G, L, M), gy (B, Cout, L, M) complex64 on the CPU; ref: dict of complex128 y, gx, gw"""
    from makani_amd import ops
    B, cin = x.shape[:2]
    cout = gy.shape[1]
    T, gS, gw = _diag_raw(ops.complex_to_s(x.to(DEV)), w, ops.complex_to_s(gy.to(DEV)), B, tri_off)
    assert T.shape[-1] == B * ops.round4(cout) and gS.shape[-1] == B * ops.round4(cin)
    assert _pad_is_zero(T, B, cout) and _pad_is_zero(gS, B, cin)              # channels [C, round4(C)) of both outputs
    e = (_report("diag-fwd", _unmasked(T, B, cout), ref["y"].reshape(B, cout, *x.shape[-2:])),
         _report("diag-dgrad", _unmasked(gS, B, cin), ref["gx"].reshape(x.shape)),
         _report("diag-wgrad", gw, ref["gw"]))
    assert max(e) < GATE, e
    return T, gS, gw


def _check_sep(x, w3, gy, tri_off, ref):
    """x, gy (B, C, L, M), w3 (C, L, Mw) complex64 on the CPU"""
    from makani_amd import ops
    B, Cc = x.shape[:2]
    y, gS, gw = _sep_raw(ops.complex_to_s(x.to(DEV)), w3, ops.complex_to_s(gy.to(DEV)), B, tri_off)
    assert _pad_is_zero(y, B, Cc) and _pad_is_zero(gS, B, Cc)
    e = (_report("sep-mul", _unmasked(y, B, Cc), ref["y"].reshape(x.shape)),
         _report("sep-conjmul", _unmasked(gS, B, Cc), ref["gx"].reshape(x.shape)),
         _report("sep-wgrad", gw, ref["gw"].reshape(w3.shape)))
    assert max(e) < GATE, e
    return y, gS, gw


# --------------------------------------------------------------------------- #
# problems
# --------------------------------------------------------------------------- #
GLOBAL = (24, 25)                 # the global spectrum the shard cases are cut from
# (l0, L, m0, M): tri_off = l0 - m0
SHARDS = {"live+12": (12, 12, 0, 13), "dead-13": (0, 12, 13, 12), "deadrows-3": (6, 6, 9, 8), "ragged-1": (12, 12, 13, 12)}


def _diag_problem(B, G, cgi, cgo, L, M, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + 17 * cgi + cgo)
    x = _randc(gen, B, G, cgi, L, M)
    w = _randc(gen, G, cgi, cgo, L, M) / cgi ** 0.5
    gy = _randc(gen, B, G, cgo, L, M)
    return x, w, gy


def _sep_problem(B, Cc, L, M, Mw, seed=0):
    gen = torch.Generator().manual_seed(2000 * seed + 13 * Cc + Mw)
    x = _randc(gen, B, 1, Cc, L, M)
    w = _randc(gen, 1, Cc, L, M) if Mw == M else _randc(gen, 1, Cc, L)         # 1 / sqrt(Cin / G) = 1: one channel per product
    gy = _randc(gen, B, 1, Cc, L, M)
    return ("sep_lmwise" if Mw == M else "sep_lwise"), x, w, gy


def _flat(t):
    """(B, G, C/G, L, M) -> (B, C, L, M)"""
    return t.reshape(t.shape[0], -1, *t.shape[-2:])


DIAG_CASES = [
    # (B, G, Cin/G, Cout/G, L, M)
    pytest.param(3, 1, 70, 37, 9, 10, id="k70-n37-3stages-3blocks-b3"),
    pytest.param(1, 1, 32, 16, 5, 6, id="k32-n16-exact-tiles"),
    pytest.param(1, 1, 33, 17, 5, 6, id="k33-n17-one-past-pad-in-2nd-block"),
    pytest.param(2, 1, 7, 5, 8, 8, id="k7-n5-idle-waves-lm64"),
    pytest.param(2, 3, 11, 6, 9, 10, id="g3-k11-n6-unaligned-slices"),
    pytest.param(2, 2, 3, 5, 12, 12, id="g2-k3-n5-golden-shape"),
]


@pytest.mark.parametrize("B,G,cgi,cgo,L,M", DIAG_CASES)
def test_diag_kernels_at_tile_edges(B, G, cgi, cgo, L, M):
    x, w, gy = _diag_problem(B, G, cgi, cgo, L, M)
    gx, gw = R.tri_grads("lmwise", x, w, gy)
    ref = dict(y=R.tri_contract("lmwise", x, w), gx=gx, gw=gw)
    assert (ref["y"][..., _dead(L, M, 0)] == 0).all() and (ref["gw"][..., _dead(L, M, 0)] == 0).all()
    _check_diag(_flat(x), w, _flat(gy), 0, ref)


@pytest.mark.parametrize("key", list(SHARDS))
def test_diag_kernels_on_a_shard_of_a_global_spectrum(key):
    """(B, G, Cin, Cout) = (2, 1, 9, 18): one rank's window of a 24 x 25 spectrum, tri_off = l0 - m0"""
    l0, L, m0, M = SHARDS[key]
    x, w, gy = _diag_problem(2, 1, 9, 18, *GLOBAL, seed=1)
    s = R.shard("lmwise", x, w, gy, l0, L, m0, M)
    T, gS, gw = _check_diag(_flat(s["x"]).contiguous(), s["w"].contiguous(), _flat(s["gy"]).contiguous(), l0 - m0, s)
    dead = _dead(L, M, l0 - m0)
    assert torch.equal(dead, ~R.live(*GLOBAL)[l0:l0 + L, m0:m0 + M])
    assert (T[dead.to(DEV)] == 0).all() and (gS[dead.to(DEV)] == 0).all() and (gw[..., dead.to(DEV)] == 0).all()
    if key == "dead-13":            # no live position at all: nothing but zeros anywhere
        assert dead.all() and not T.any() and not gS.any() and not torch.view_as_real(gw).any()
    if key == "live+12":
        assert not dead.any()
    if key == "deadrows-3":
        assert dead[:3].all() and not dead[3:, 0].any() and dead[3:].any()


SEP_SHAPES = [
    pytest.param(2, 7, 9, 10, id="c7-pad8"),
    pytest.param(3, 33, 16, 17, id="c33-b3"),
    pytest.param(1, 4, 5, 6, id="c4"),
    pytest.param(1, 1022, 64, 65, id="c1022-grid-stride"),
]


@pytest.mark.parametrize("form", ["lm", "l"])
@pytest.mark.parametrize("B,Cc,L,M", SEP_SHAPES)
def test_sep_kernels(B, Cc, L, M, form):
    Mw = M if form == "lm" else 1
    name, x, w, gy = _sep_problem(B, Cc, L, M, Mw)
    if Cc == 1022:                  # more four-channel items than 4096 workgroups of 256 hold: the grid-stride loop
        assert L * M * B * ((Cc + 3) // 4) > 4096 * 256
    gx, gw = R.tri_grads(name, x, w, gy)
    _check_sep(_flat(x), w.reshape(Cc, L, Mw), _flat(gy), 0, dict(y=R.tri_contract(name, x, w), gx=gx, gw=gw))


@pytest.mark.parametrize("form", ["lm", "l"])
@pytest.mark.parametrize("key", list(SHARDS))
def test_sep_kernels_on_a_shard_of_a_global_spectrum(key, form):
    """C = 6, B = 2; the l-wise weight has no m axis, so only l is cut and the weight gradient is the partial sum over the
    window's own live orders"""
    l0, L, m0, M = SHARDS[key]
    Mw = M if form == "lm" else 1
    name, x, w, gy = _sep_problem(2, 6, *GLOBAL, GLOBAL[1] if form == "lm" else 1, seed=1)
    s = R.shard(name, x, w, gy, l0, L, m0, M)
    y, gS, gw = _check_sep(_flat(s["x"]).contiguous(), s["w"].reshape(6, L, Mw).contiguous(), _flat(s["gy"]).contiguous(), l0 - m0, s)
    dead = _dead(L, M, l0 - m0).to(DEV)
    assert (y[dead] == 0).all() and (gS[dead] == 0).all()
    if form == "lm":
        assert (gw[:, dead] == 0).all()
    if key == "dead-13":
        assert not y.any() and not gS.any() and not torch.view_as_real(gw).any()
    if key == "deadrows-3" and form == "l":
        assert not torch.view_as_real(gw[:, :3]).any() and torch.view_as_real(gw[:, 3:]).all()    # rows without a live order


# --------------------------------------------------------------------------- #
# contract 1: nothing is read at dead positions
# --------------------------------------------------------------------------- #
def _poisoned(S, tri_off):
    L, M = S.shape[:2]
    P = S.clone()
    P[_dead(L, M, tri_off).to(S.device)] = float("nan")           # both parts, every row: real channels and padding alike
    return P


@pytest.mark.parametrize("family", ["diag", "sep-lm", "sep-l"])
def test_dead_positions_are_never_read(family):
    """NaN at every dead position (m > l + tri_off) of the input and of the cotangent, after complex_to_s: all outputs and
    gradients stay finite, equal the un-poisoned run bit for bit, and are exact zeros at the dead positions"""
    from makani_amd import ops
    l0, L, m0, M = SHARDS["deadrows-3"]
    tri_off, B = l0 - m0, 2
    if family == "diag":
        x, w, gy = _diag_problem(B, 1, 9, 18, L, M, seed=2)
        w_arg, run = w, _diag_raw
    else:
        Mw = M if family == "sep-lm" else 1
        _, x, w, gy = _sep_problem(B, 6, L, M, Mw, seed=2)
        w_arg, run = w.reshape(6, L, Mw), _sep_raw
    S, gT = ops.complex_to_s(_flat(x).to(DEV)), ops.complex_to_s(_flat(gy).to(DEV))
    Sp, gTp = _poisoned(S, tri_off), _poisoned(gT, tri_off)
    dead = _dead(L, M, tri_off).to(DEV)
    assert torch.isnan(Sp[dead]).all() and torch.isfinite(Sp[~dead]).all() and torch.equal(Sp[~dead], S[~dead])
    clean, pois = run(S, w_arg, gT, B, tri_off), run(Sp, w_arg, gTp, B, tri_off)
    for a, b in zip(clean, pois):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
        assert torch.isfinite(b).all() and torch.equal(a, b)
    assert (pois[0][dead] == 0).all() and (pois[1][dead] == 0).all() and pois[0][~dead].any()
    if family != "sep-l":
        assert (pois[2][..., dead] == 0).all()


# --------------------------------------------------------------------------- #
# contract 2: nothing is written outside the output
# --------------------------------------------------------------------------- #
GUARD, SENTINEL = 256, -777.25


class _Carved:
    """an n-float output in the middle of a sentinel-filled buffer, GUARD floats on either side"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def check(self, expect):
        torch.cuda.synchronize()
        e = torch.view_as_real(expect) if expect.is_complex() else expect
        assert e.numel() == self.n
        assert (self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + self.n:] == SENTINEL).all()
        assert torch.equal(self.buf[GUARD:GUARD + self.n], e.reshape(-1))         # ... and the call did its work


def test_diag_entry_points_stay_inside_their_output():
    from makani_amd import ops
    from makani_amd._lib import lib, check, ptr, stream
    B, cin, cout, L, M = 1, 33, 17, 5, 6
    cip, cop = ops.round4(cin), ops.round4(cout)
    x, w, gy = _diag_problem(B, 1, cin, cout, L, M, seed=3)
    S, gT = ops.complex_to_s(_flat(x).to(DEV)), ops.complex_to_s(_flat(gy).to(DEV))
    T, gS, gw = _diag_raw(S, w, gT, B, 0)
    wr = torch.view_as_real(w[0].to(DEV).contiguous())
    out = _Carved(L * M * 2 * B * cop)
    check(lib().mk_spec_diag_apply(ptr(S), ptr(wr), out.ptr, L, M, B, cin, cout, cip, cop, cop - cout, 0, 0, stream()), "diag fwd")
    out.check(T)
    assert (out.buf[GUARD:GUARD + out.n].view(L, M, 2, B, cop)[..., cout:] == 0).all()       # the padding 17 -> 20 is written, as zeros
    out = _Carved(L * M * 2 * B * cip)
    check(lib().mk_spec_diag_apply(ptr(gT), ptr(wr), out.ptr, L, M, B, cin, cout, cop, cip, cip - cin, 0, 1, stream()), "diag dgrad")
    out.check(gS)
    out = _Carved(cin * cout * L * M * 2)
    check(lib().mk_spec_diag_wgrad(ptr(S), ptr(gT), out.ptr, L, M, B, cin, cout, cip, cop, 0, stream()), "diag wgrad")
    out.check(gw)


@pytest.mark.parametrize("form", ["lm", "l"])
def test_sep_entry_points_stay_inside_their_output(form):
    from makani_amd import ops
    from makani_amd._lib import lib, check, ptr, stream
    B, Cc, L, M = 2, 7, 9, 10
    Mw, Cp = (M if form == "lm" else 1), ops.round4(Cc)
    _, x, w, gy = _sep_problem(B, Cc, L, M, Mw, seed=3)
    S, gT = ops.complex_to_s(_flat(x).to(DEV)), ops.complex_to_s(_flat(gy).to(DEV))
    Ws = ops.complex_to_s(w.reshape(1, Cc, L, Mw).to(DEV))
    S1, Ws1 = S.clone().requires_grad_(True), Ws.clone().requires_grad_(True)
    y = ops.SepContractFn.apply(S1, Ws1, B, 0)
    y.backward(gT)
    out = _Carved(L * M * 2 * B * Cp)
    check(lib().mk_spec_sep_mul(ptr(S), ptr(Ws), out.ptr, L, M, Mw, B, Cp, 0, 0, stream()), "sep mul")
    out.check(y.detach())
    out = _Carved(L * M * 2 * B * Cp)
    check(lib().mk_spec_sep_mul(ptr(gT), ptr(Ws), out.ptr, L, M, Mw, B, Cp, 0, 1, stream()), "sep conj-mul")
    out.check(S1.grad)
    out = _Carved(L * Mw * 2 * Cp)
    check(lib().mk_spec_sep_wgrad(ptr(S), ptr(gT), out.ptr, L, M, Mw, B, Cp, 0, stream()), "sep wgrad")
    out.check(Ws1.grad)


# --------------------------------------------------------------------------- #
# module level, larger than one tile: ma.SpectralConv against the restated reference module
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("op,separable,G,cin,cout", [
    pytest.param("diagonal", False, 1, 40, 36, id="diagonal-g1-40to36"),
    pytest.param("diagonal", False, 2, 34, 18, id="diagonal-g2-34to18"),
    pytest.param("diagonal", True, 1, 33, 33, id="diagonal-sep-33"),
    pytest.param("dhconv", True, 3, 33, 33, id="dhconv-sep-g3-33"),
])
def test_spectral_conv_beyond_one_tile_matches_restated_reference(op, separable, G, cin, cout):
    """(33, 64) equiangular, lmax = mmax = 16 (the reference's "diagonal" initialisation broadcasts its per-l scale against the
    m axis): forward, input gradient and weight gradient against oracle.sfno.SpectralConv holding the same weight"""
    import makani_amd as ma
    from oracle import sfno as osf
    from oracle import sht as osht
    kw = dict(lmax=16, mmax=16, grid="equiangular")
    torch.manual_seed(40 + cin)
    layer = ma.SpectralConv(ma.RealSHT(33, 64, **kw), ma.InverseRealSHT(33, 64, **kw), cin, cout, num_groups=G, operator_type=op,
                            separable=separable).to(DEV)
    ref = osf.SpectralConv(osht.RealSHT(33, 64, **kw).float(), osht.InverseRealSHT(33, 64, **kw).float(), cin, cout, num_groups=G,
                           operator_type=op, separable=separable)
    assert ref.weight.shape == layer.weight.shape
    with torch.no_grad():
        ref.weight.copy_(layer.weight.cpu())
    x = torch.randn(2, cin, 33, 64)
    gy = torch.randn(2, cout, 33, 64)
    xr = x.clone().requires_grad_(True)
    yr, _ = ref(xr)
    (yr * gy).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    yd, _ = layer(xd)
    (yd * gy.to(DEV)).sum().backward()
    e = rel_l2(yd, yr), rel_l2(xd.grad, xr.grad), rel_l2(layer.weight.grad, ref.weight.grad)
    print(f"specpw module {op} sep={separable} G={G}: y {e[0]:.2e} gx {e[1]:.2e} gw {e[2]:.2e}", flush=True)
    assert e[0] < TOL_OP and e[1] < 2 * TOL_OP and e[2] < 2 * TOL_OP, e
