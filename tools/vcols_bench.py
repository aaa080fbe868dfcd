"""mk_vcols_repack against the torch narrow / contiguous / cat / pad expressions it replaces, HIP events, at the full-size h2 w2
shard shapes (721 x 1440, L = M = 721) for 2 members x 14 wind pairs = 28 pairs (docs/LAB_NOTEBOOK.md 6.13,
profiles/vcols_repack_bench.txt).  usage: python tools/vcols_bench.py [file to write the lines to]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from makani_amd import ops  # noqa: E402

dev = "cuda"
OUT = sys.argv[1] if len(sys.argv) > 1 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


M, hl, Mloc, nlat, P, Pw = 721, 361, 361, 721, 28, 14
Rp, Rpw = ops.round32(P), ops.round32(Pw)
blocks = 4

# ---- exchange 2 of the analysis, (w) m <-> pairs: F (M, hl, 2, 2 round32(P_w)) -> (M_loc, hl, 2, 2 round32(P))
F = torch.randn(M, hl, blocks, Rpw, device=dev)
F[..., Pw:] = 0
m0 = 361                                        # the peer's order range [361, 721)
n_m = M - m0
slab = torch.empty(n_m, hl, blocks, Pw, device=dev)


def pack_kernel():
    ops.vcols_repack(F.narrow(0, m0, n_m), slab, Pw, 0, 0, False)


def pack_torch():
    return F.narrow(0, m0, n_m)[..., :Pw].contiguous()


assert torch.equal(pack_torch(), (pack_kernel(), slab)[1])
nbytes = 2 * slab.numel() * 4
for name, fn in (("pack   kernel", pack_kernel), ("pack   torch narrow+contiguous", pack_torch), ("pack   kernel (again)", pack_kernel)):
    med, lo, hi = timed(fn)
    say(f"{name:40s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / 1e6:.1f} MB moved  {nbytes / med / 1e6:.0f} GB/s")

own = torch.randn(Mloc, hl, blocks, Rpw, device=dev)          # this rank's own share, still in the padded FFT output
arrived = torch.randn(Mloc, hl, blocks, Pw, device=dev)       # the peer's slab
y = torch.empty(Mloc, hl, blocks, Rp, device=dev)


def unpack_kernel():
    ops.vcols_repack(own, y, Pw, 0, 0, False)
    ops.vcols_repack(arrived, y, Pw, 0, Pw, True)


def unpack_torch():
    return torch.nn.functional.pad(torch.cat([own[..., :Pw], arrived], dim=3), (0, Rp - P))


unpack_kernel()
assert torch.equal(unpack_torch(), y)
nbytes = (2 * Mloc * hl * blocks * P + Mloc * hl * blocks * (Rp - P)) * 4
for name, fn in (("unpack kernel (2 launches)", unpack_kernel), ("unpack torch cat+pad", unpack_torch), ("unpack kernel (again)", unpack_kernel)):
    med, lo, hi = timed(fn)
    say(f"{name:40s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / 1e6:.1f} MB moved  {nbytes / med / 1e6:.0f} GB/s")

# ---- exchange 3, (h) pairs <-> lat: (M_loc, hl, 2, 2 round32(P)) -> (M_loc, nlat, 2, 2 round32(P_h)); slabs land in latitude ranges
Ph = 14
Rph = ops.round32(Ph)
src = torch.randn(Mloc, hl, blocks, Rp, device=dev)
arrived = torch.randn(Mloc, nlat - hl, blocks, Ph, device=dev)
y2 = torch.empty(Mloc, nlat, blocks, Rph, device=dev)


def unpack2_kernel():
    ops.vcols_repack(src, y2.narrow(1, 0, hl), Ph, 0, 0, True)
    ops.vcols_repack(arrived, y2.narrow(1, hl, nlat - hl), Ph, 0, 0, True)


def unpack2_torch():
    return torch.nn.functional.pad(torch.cat([src[..., :Ph], arrived], dim=1), (0, Rph - Ph))


unpack2_kernel()
assert torch.equal(unpack2_torch(), y2)
nbytes = (2 * Mloc * nlat * blocks * Ph + Mloc * nlat * blocks * (Rph - Ph)) * 4
for name, fn in (("unpack(lat) kernel (2 launches)", unpack2_kernel), ("unpack(lat) torch cat+pad", unpack2_torch),
                 ("unpack(lat) kernel (again)", unpack2_kernel)):
    med, lo, hi = timed(fn)
    say(f"{name:40s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / 1e6:.1f} MB moved  {nbytes / med / 1e6:.0f} GB/s")

# ---- the 16-byte path: 16 pairs per share (every extent a multiple of 4)
slab16 = torch.empty(n_m, hl, blocks, 16, device=dev)
med, lo, hi = timed(lambda: ops.vcols_repack(F.narrow(0, m0, n_m), slab16, 16, 0, 0, False))
nbytes = 2 * slab16.numel() * 4
say(f"{'pack   kernel, 16 pairs (16-byte path)':40s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / 1e6:.1f} MB moved  {nbytes / med / 1e6:.0f} GB/s")
med, lo, hi = timed(lambda: F.narrow(0, m0, n_m)[..., :16].contiguous())
say(f"{'pack   torch, 16 pairs':40s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / 1e6:.1f} MB moved  {nbytes / med / 1e6:.0f} GB/s")

if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
