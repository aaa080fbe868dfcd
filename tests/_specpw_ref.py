"""complex128 restatement of the four grouped spectral contractions of makani/models/common/contractions.py:17-54, written as
plain ``torch.einsum`` on the CPU, with their gradients for a given cotangent and the triangle rule of a (possibly sharded)
spectrum.  x (B, G, I, L, M); cotangent and result shaped like the output.

  "lmwise"      bgixy,gioxy->bgoxy    w (G, I, O, L, M)     the "diagonal" operator
  "lwise"       bgixy,giox->bgoxy     w (G, I, O, L)        "dhconv"
  "sep_lmwise"  bgixy,gixy->bgixy     w (G, I, L, M)        separable "diagonal"
  "sep_lwise"   bgixy,gix->bgixy      w (G, I, L)           separable "dhconv"

Gradients follow torch's convention for a real loss of complex tensors: gx = gy . conj(w), gw = conj(x) . gy, summed over
whatever the forward broadcasts (b always; m as well for the two l-wise weights).

Triangle rule: position (l, m) of a shard whose first degree / order are (l0, m0) is live iff m + m0 <= l + l0.  A dead
position holds no coefficient: it contributes nothing, and the result and both gradients are exact zeros there.  Test helper."""
import torch

FWD = {"lmwise": "bgixy,gioxy->bgoxy", "lwise": "bgixy,giox->bgoxy", "sep_lmwise": "bgixy,gixy->bgixy", "sep_lwise": "bgixy,gix->bgixy"}
DGRAD = {"lmwise": "bgoxy,gioxy->bgixy", "lwise": "bgoxy,giox->bgixy", "sep_lmwise": "bgixy,gixy->bgixy", "sep_lwise": "bgixy,gix->bgixy"}
WGRAD = {"lmwise": "bgixy,bgoxy->gioxy", "lwise": "bgixy,bgoxy->giox", "sep_lmwise": "bgixy,bgixy->gixy", "sep_lwise": "bgixy,bgixy->gix"}
LWISE = ("lwise", "sep_lwise")          # weights without an m axis


def c128(t):
    return t.detach().cpu().to(torch.complex128)


def contract(name, x, w):
    """the plain contraction, no triangle"""
    return torch.einsum(FWD[name], c128(x), c128(w))


def grads(name, x, w, gy):
    """(gx, gw) of Re sum(conj(gy) * contract(x, w)), no triangle"""
    x, w, gy = c128(x), c128(w), c128(gy)
    return torch.einsum(DGRAD[name], gy, w.conj()), torch.einsum(WGRAD[name], x.conj(), gy)


def live(L, M, l0=0, m0=0):
    """(L, M) bool: m + m0 <= l + l0"""
    return torch.arange(M)[None, :] + m0 <= torch.arange(L)[:, None] + l0


def tri_contract(name, x, w, l0=0, m0=0):
    """the contraction of a spectrum that only exists at its live positions"""
    x = c128(x)
    return contract(name, x * live(*x.shape[-2:], l0, m0), w)


def tri_grads(name, x, w, gy, l0=0, m0=0):
    """(gx, gw) under the triangle rule: dead positions of x and of the cotangent do not exist (the contractions are pointwise
    in (l, m), so both gradients come out as exact zeros there)"""
    x, gy = c128(x), c128(gy)
    mask = live(*x.shape[-2:], l0, m0)
    return grads(name, x * mask, w, gy * mask)


def _cut(t, has_m, l0, L, m0, M):
    return t[..., l0:l0 + L, m0:m0 + M] if has_m else t[..., l0:l0 + L]


def shard(name, x, w, gy, l0, L, m0, M):
    """what the rank that owns degrees [l0, l0 + L) and orders [m0, m0 + M) of a GLOBAL problem holds and must compute.
    x (B, G, I, Lg, Mg), w and the cotangent gy are global; the global complex128 result is computed once and cut.  The
    gradients are those of the global contraction for the cotangent restricted to the rank's window, so an l-wise weight
    gradient is the rank's partial sum over its own orders (what it holds before the reduction over the "w" group).
    Returns a dict of the local x, w, gy (as given, uncut in value: dead positions keep whatever they held) and the local
    complex128 y, gx, gw."""
    x128, gy128 = c128(x), c128(gy)
    win = torch.zeros(x128.shape[-2:], dtype=torch.bool)
    win[l0:l0 + L, m0:m0 + M] = True
    y = tri_contract(name, x128, w)
    gx, gw = tri_grads(name, x128, w, gy128 * win)
    has_m = name not in LWISE
    return dict(x=x[..., l0:l0 + L, m0:m0 + M], w=_cut(w, has_m, l0, L, m0, M), gy=gy[..., l0:l0 + L, m0:m0 + M],
                y=y[..., l0:l0 + L, m0:m0 + M], gx=gx[..., l0:l0 + L, m0:m0 + M], gw=_cut(gw, has_m, l0, L, m0, M))
