"""Pin tests/_specpw_ref.py (the complex128 restatement the GPU sweep of csrc/spectral_pointwise.hip is measured against) to
the reference's own ``_contract_dense_pytorch`` (fixtures of oracle/make_golden.py::contraction_fixtures) and to autograd."""
import pytest
import torch

import _specpw_ref as R
from conftest import load_golden, rel_l2

TOL = 1e-6                    # the fixtures are complex64


def test_restatement_matches_reference_contractions():
    g = load_golden("contractions.npz")
    x, w, wd = (torch.from_numpy(g[k]) for k in ("x", "w", "wd"))
    assert rel_l2(R.contract("lwise", x, w), torch.from_numpy(g["y"]).to(torch.complex128)) < TOL
    assert rel_l2(R.contract("lmwise", x, wd), torch.from_numpy(g["yd"]).to(torch.complex128)) < TOL


def test_restatement_matches_reference_separable_and_grouped_contractions():
    g = load_golden("contractions_sep.npz")
    t = {k: torch.from_numpy(g[k]) for k in g.files}
    assert t["xg"].shape[1] == 2 and t["wg"].shape[0] == 2                          # the grouped case is grouped
    for name, x, w, y in (("sep_lmwise", "xs", "ws_lm", "ys_lm"), ("sep_lwise", "xs", "ws_l", "ys_l"), ("lmwise", "xg", "wg", "yg")):
        assert t[y].dtype == torch.complex64 and t[y].abs().max() > 0
        assert rel_l2(R.contract(name, t[x], t[w]), t[y].to(torch.complex128)) < TOL, name


def _problem(name, B=2, G=2, I=3, O=4, L=7, M=9, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.complex128, generator=gen)
    sep = name.startswith("sep")
    w_shape = [G, I] + ([] if sep else [O]) + [L] + ([] if name in R.LWISE else [M])
    return rn(B, G, I, L, M), rn(*w_shape), rn(B, G, I if sep else O, L, M)


@pytest.mark.parametrize("name", list(R.FWD))
def test_gradients_match_autograd(name):
    """the closed forms gx = gy conj(w), gw = conj(x) gy are what torch differentiates the einsum to, with and without the
    triangle (there: x exists only at live positions)"""
    x, w, gy = _problem(name)
    for l0, m0 in ((None, None), (0, 0), (3, 5)):
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        if l0 is None:
            y = torch.einsum(R.FWD[name], xa, wa)
            gx, gw = R.grads(name, x, w, gy)
            assert torch.equal(y.detach(), R.contract(name, x, w))
        else:
            y = torch.einsum(R.FWD[name], xa * R.live(*x.shape[-2:], l0, m0), wa)
            gx, gw = R.tri_grads(name, x, w, gy, l0, m0)
            assert torch.equal(y.detach(), R.tri_contract(name, x, w, l0, m0))
        torch.view_as_real(y.conj() * gy)[..., 0].sum().backward()                  # Re <gy, y>
        assert rel_l2(gx, xa.grad) < 1e-14 and rel_l2(gw, wa.grad) < 1e-14


def test_triangle_rule():
    m = R.live(4, 5)
    assert m.tolist() == [[True, False, False, False, False], [True, True, False, False, False],
                          [True, True, True, False, False], [True, True, True, True, False]]
    assert R.live(3, 3, l0=2, m0=0).all() and not R.live(3, 3, l0=0, m0=3).any()
    assert torch.equal(R.live(6, 8, l0=6, m0=9), R.live(24, 25)[6:12, 9:17])       # a shard's rule is the global rule, cut


@pytest.mark.parametrize("name", list(R.FWD))
def test_dead_positions_are_exact_zeros(name):
    x, w, gy = _problem(name)
    dead = ~R.live(*x.shape[-2:], 2, 4)
    assert dead.any() and (~dead).any()
    y = R.tri_contract(name, x, w, 2, 4)
    gx, gw = R.tri_grads(name, x, w, gy, 2, 4)
    assert (y[..., dead] == 0).all() and (gx[..., dead] == 0).all()
    assert (y[..., ~dead] != 0).all() and (gx[..., ~dead] != 0).all()
    if name not in R.LWISE:
        assert (gw[..., dead] == 0).all() and (gw[..., ~dead] != 0).all()


@pytest.mark.parametrize("name", list(R.FWD))
def test_unsharded_shard_is_the_restatement(name):
    x, w, gy = _problem(name, L=7, M=9)
    s = R.shard(name, x, w, gy, 0, 7, 0, 9)
    gx, gw = R.tri_grads(name, x, w, gy)
    assert torch.equal(s["x"], x) and torch.equal(s["w"], w) and torch.equal(s["gy"], gy)
    assert torch.equal(s["y"], R.tri_contract(name, x, w)) and torch.equal(s["gx"], gx) and torch.equal(s["gw"], gw)


@pytest.mark.parametrize("name", list(R.FWD))
def test_shard_is_the_local_problem_with_offsets(name):
    """a rank's window of the global result is the local contraction of the local slices under the shifted triangle, and the
    four windows of an h2 x w2 split tile the global gradients (the l-wise weight gradient as a sum over the w ranks)"""
    x, w, gy = _problem(name, L=10, M=11)
    gxg, gwg = R.tri_grads(name, x, w, gy)
    gw_sum = torch.zeros_like(gwg)
    for l0, L in ((0, 5), (5, 5)):
        for m0, M in ((0, 6), (6, 5)):
            s = R.shard(name, x, w, gy, l0, L, m0, M)
            assert rel_l2(s["y"], R.tri_contract(name, s["x"], s["w"], l0, m0)) < 1e-15
            gx, gw = R.tri_grads(name, s["x"], s["w"], s["gy"], l0, m0)
            assert rel_l2(s["gx"], gx) < 1e-15 and rel_l2(s["gw"], gw) < 1e-15
            assert rel_l2(s["gx"], gxg[..., l0:l0 + L, m0:m0 + M]) < 1e-15
            if name in R.LWISE:
                gw_sum[..., l0:l0 + L] += s["gw"]
            else:
                gw_sum[..., l0:l0 + L, m0:m0 + M] += s["gw"]
    assert rel_l2(gw_sum, gwg) < 1e-15
