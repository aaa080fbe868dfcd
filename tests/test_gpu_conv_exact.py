"""The bf16 channel GEMMs (csrc/conv1x1.hip) element for element on exact integer data.

A bf16 GEMM with fp32 accumulation is exact on small integers in any summation order: with x in {-1, 0, 1}, w in {-1, 0, 1} / 8
and every sum a multiple of 1/8 below 32, the fp32 accumulator holds the exact value whatever order the tiles, k-steps and splits
run in, and the bf16 rounding of the result is the identity.  So the expected output is ONE tensor for every kernel form, tile
height, store policy and split count, and the comparison is equality over every element.  That makes the matrix below a detector
for indexing faults (a stale ring slot, a slab row stored one row too far, a ragged tail read past its end), which the rel-L2
gates of tests/test_gpu_kernels.py cannot see; rounding behaviour stays with those tests.

Conventions:
  * the C ABI is called directly, so the test owns every buffer;
  * every output (Y, Ypre, dW, db, the split workspace) is an interior slice of a larger buffer filled with a sentinel that no
    result can take, refilled before EACH call: an element the kernel did not write cannot compare equal, and after the call
    every guard element (256 KiB on either side) must still hold the sentinel;
  * every operand is an interior slice of a buffer filled with NaN (the weight block's pad columns K .. lda - 1 are zero, as
    its contract says): whatever a kernel lets in from outside an operand turns a stored value into a NaN.
Nothing here reads or writes outside the test's own allocations; the launches are the ones the product makes.

The case tables are plain data and importable without a GPU: tests/test_conv_exact_cases.py checks on the CPU, against
csrc/conv1x1_plan.h itself, that every kernel, template variant, tile height and reducer is reached by them."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD_BYTES = 256 * 1024
SENT_BF16 = -12288.0            # 0xC640: finite, and no output below is 32 or more in magnitude
SENT_F32 = -(2.0 ** 100)        # finite, and every weight-gradient sum is an integer below 2^24

# ---- the case tables ------------------------------------------------------------------------------------------------
# forward / data gradient: (family, B, M, K, N, long_stream).  `family` is the kernel the PLAIN call runs with the switches unset
# (checked by tests/test_conv_exact_cases.py); lda = K rounded up to a multiple of 8.
FWD_CASES = [
    # tile kernel
    ("tile", 1, 5, 3, 8, False),                    # one 16-byte vector, K below one k16-step
    ("tile", 2, 129, 72, 136, False),               # 128 + 1 rows, 64 + 8 k, 128 + 8 pixels, batch
    ("tile", 1, 200, 40, 264, False),               # K < 64
    ("tile", 1, 300, 384, 56, False),               # N < 64 keeps a K = 384 shape off the stationary kernels; six k-tiles
    ("tile", 1, 73, 72, 524296, False),             # the 128 x 256 form (N >= 2^19), ragged last tile
    # 73-channel stationary kernel
    ("astat73", 1, 256, 73, 64, False),             # slab with rows past M, one tile
    ("astat73", 2, 385, 80, 72, False),             # second slab of one row, K = lda, ragged 8 pixels, batch
    ("astat73", 1, 256, 73, 264, False),            # pre-activation AND an operand: ring kernel, ragged second k-tile
    ("astat73", 1, 256, 77, 327752, True),          # >= 10 tiles per workgroup against a ring of 5 / 8 slots
    # two-group stationary kernel, K = 384
    ("astat2", 1, 256, 384, 64, False),
    ("astat2", 2, 385, 384, 72, False),
    ("astat2", 1, 768, 384, 328, False),
    ("astat2", 1, 384, 384, 32776, False),          # above small_ring
    ("ring", 1, 384, 384, 32768, False),            # at small_ring: the ring kernel without a stored pre-activation
    ("astat2", 1, 300, 384, 98312, True),           # six tiles per stream against a 4-slot ring
    # ring kernel
    ("ring", 1, 192, 64, 256, False),               # one tile, one k-tile: the second stage is never requested
    ("ring", 2, 193, 72, 264, False),               # 192-row tiles, the second of one row
    ("ring", 1, 256, 128, 520, False),              # 256-row tiles
    ("ring", 1, 577, 200, 256, False),              # 256-row tiles, the last of 65 rows, ragged fourth k-tile
    ("ring", 1, 384, 768, 65544, False),            # 257 tiles: plain / + bias on the 384-row tile, a workgroup with two tiles
    ("ring", 1, 192, 128, 196616, True),            # three and four tiles per workgroup against two stages
]

# name: (bias, act, stored pre-activation, R, G)
VARIANTS = {
    "plain": (False, False, False, False, False),
    "bias": (True, False, False, False, False),
    "bias_gelu_pre": (True, True, True, False, False),
    "bias_gelu": (True, True, False, False, False),
    "res": (False, False, False, True, False),
    "bias_gelu_pre_res": (True, True, True, True, False),
    "dgelu": (False, False, False, False, True),
    "dgelu_res": (False, False, False, True, True),
}

# weight gradient: (family, B, M, K, N)
WG_CASES = [
    ("tile", 1, 5, 3, 8),
    ("tile", 2, 129, 130, 136),
    ("tile", 1, 64, 64, 4104),                      # three splits, reduce_splits4
    ("ring", 1, 97, 9, 2048),                       # P = X; M K odd: the scalar reduce_splits
    ("ring", 1, 9, 97, 2056),                       # P = G, ragged pixels
    ("ring", 2, 384, 384, 8200),                    # two 192-row slabs, batch, 34 splits: both loops of the reducer
    ("ring", 1, 385, 384, 2048),                    # 256-row slabs, the second of 129
    ("ring", 1, 384, 449, 2048),
    ("ring", 1, 449, 400, 2048),                    # two 384-row slabs of Q, either operand as Q
    ("ring", 1, 400, 449, 2048),
]
# accumulate = 1: one tile-kernel case (reduce_splits4) and one ring-kernel case (the scalar reducer)
WG_ACCUMULATE = [("tile", 1, 64, 64, 4104), ("ring", 1, 97, 9, 2048)]


def round8(k):
    return (k + 7) // 8 * 8


def fwd_id(case):
    fam, B, M, K, N, long_stream = case
    return f"{fam}-{B}x{M}x{K}x{N}" + ("-longstream" if long_stream else "")


def wg_id(case):
    return "{}-{}x{}x{}x{}".format(*case)


# ---- comparison helpers (run on any device: tests/test_conv_exact_cases.py exercises them on the CPU) -----------------------
def first_mismatches(bad, got, want, limit=8):
    """(count, [(b, m, n, got, want), ...]) of the elements flagged in ``bad`` (B, M, N), in memory order"""
    count = int(bad.sum())
    if count == 0:
        return 0, []
    idx = bad.reshape(-1).nonzero().reshape(-1)[:limit]
    _, Mm, Nn = bad.shape
    out = []
    for i in idx.tolist():
        b, m, n = i // (Mm * Nn), (i // Nn) % Mm, i % Nn
        out.append((b, m, n, float(got[b, m, n]), float(want[b, m, n])))
    return count, out


def describe(what, bad, got, want):
    """[] or one line naming the first mismatches as (b, m, n): got / want"""
    count, first = first_mismatches(bad, got, want)
    if count == 0:
        return []
    cells = ", ".join(f"({b}, {m}, {n}): {g!r} / {w!r}" for b, m, n, g, w in first)
    return [f"{what}: {count} of {bad.numel()} elements wrong; first (b, m, n): got / want = {cells}"]


def mismatch_exact(got, want):
    """value equality (-0 = +0) over every element; a NaN on either side is a mismatch"""
    return ~(got.double() == want.double())


def mismatch_within(got, want, tol):
    return ~((got.double() - want.double()).abs() <= tol)


def gelu_erfc(x):
    """exact GELU in fp64 without the cancellation of x (1 + erf(x / sqrt 2)) / 2 (tests/test_gpu_kernels.py: _gelu_erfc)"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def bf16_ulps(got, want):
    """distance in bf16 steps between two bf16 tensors, on their device (bit patterns are monotonic in magnitude)"""
    a = got.contiguous().view(torch.int16).to(torch.int32)
    b = want.contiguous().view(torch.int16).to(torch.int32)
    am, bm = a & 0x7FFF, b & 0x7FFF
    same_sign = ((a < 0) == (b < 0)) | ((am == 0) & (bm == 0))
    return torch.where(same_sign, (am - bm).abs(), am + bm)


def gelu_gate(what, y, pre64):
    """the gates of test_bf16_forward_gelu_is_exact_to_the_rounding_including_the_tails: at most one bf16 step from
    bf16(gelu_fp64(pre)) wherever |want| >= 1e-17, and the identical value in >= 99.9 % of those elements.  Below 1e-17 (pre = 0,
    or pre < -9 where the kernel's Phi(-9) stands in with values around 1e-18) the output must itself be below 1e-16, so that an
    unwritten element cannot hide there."""
    want = gelu_erfc(pre64).bfloat16()
    live = want.float().abs() >= 1e-17
    u = bf16_ulps(y, want)
    bad = torch.where(live, u > 1, ~(y.float().abs() <= 1e-16))
    out = describe(what + " (more than one bf16 step from gelu_fp64)", bad, y, want)
    same = float(((u == 0) & live).sum()) / max(1, int(live.sum()))
    if same < 0.999:
        out.append(f"{what}: identical to bf16(gelu_fp64) in {100 * same:.3f} % of {int(live.sum())} elements, below 99.9 %")
    return out


# ---- buffers the test owns ------------------------------------------------------------------------------------------------
class Guarded:
    """``shape`` elements as an interior slice of a larger 1-d buffer filled with ``fill``: 256 KiB on either side, the slice
    16-byte aligned (the allocation is, and the guard is a multiple of 16 bytes) and of exactly its contract size"""

    def __init__(self, shape, dtype, fill, device):
        self.n = int(math.prod(shape))
        self.g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
        self.fill = fill
        self.buf = torch.full((self.n + 2 * self.g,), fill, dtype=dtype, device=device)
        self.t = self.buf[self.g:self.g + self.n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def reset(self):
        self.buf.fill_(self.fill)

    def guards_intact(self):
        lo, hi = self.buf[:self.g], self.buf[self.g + self.n:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def operand(values, dtype):
    """``values`` as an interior slice of a NaN-filled buffer"""
    g = Guarded(tuple(values.shape), dtype, float("nan"), values.device)
    g.t.copy_(values)
    return g


def _gen(device, seed):
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    return gen


def _ints(gen, lo, hi, shape, device):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=device).double()


def forward_data(case, device):
    """the operands of one forward case as fp64 tensors holding their exact values (a seeded generator per case)"""
    _, B, M, K, N, _ = case
    gen = _gen(device, 1000 * M + K + N % 997)
    s = _ints(gen, -1, 1, (M, K), device)
    if K > 2000:                                    # thin the non-zeros so that the sums stay below 32
        s = s * (torch.rand((M, K), generator=gen, device=device) < 2000.0 / K)
    d = {
        "w": s / 8,
        "x": _ints(gen, -1, 1, (B, K, N), device),
        "bias": _ints(gen, -3, 3, (M,), device) / 4,
        "R": _ints(gen, -64, 64, (B, M, N), device) / 8,
        "G": (_ints(gen, 0, 1, (B, M, N), device) * 2 - 1) * 16,
        # the normalising operand of mk_conv1x1_nn_rnorm: per plane sc in {1, 2, -1} and sh in eighths, pb in eighths
        "sc": torch.tensor([1.0, 2.0, -1.0], dtype=torch.float64, device=device)[torch.randint(0, 3, (B, M), generator=gen, device=device)],
        "sh": _ints(gen, -8, 8, (B, M), device) / 8,
        "pb": _ints(gen, -4, 4, (M,), device) / 8,
    }
    return d


def forward_reference(d, chunk=1 << 16):
    """acc = w x in fp64 (exact), chunked over pixels"""
    B, K, N = d["x"].shape
    M = d["w"].shape[0]
    acc = torch.empty((B, M, N), dtype=torch.float64, device=d["x"].device)
    for b in range(B):
        for n0 in range(0, N, chunk):
            acc[b, :, n0:n0 + chunk] = d["w"] @ d["x"][b, :, n0:n0 + chunk]
    return acc


def exact_eighths(t):
    """the precondition on anything a forward kernel may round: a multiple of 1/8 below 32 in magnitude"""
    return bool(((t * 8) == (t * 8).round()).all()) and float(t.abs().max()) < 32.0


def rnorm_terms(d, with_pb):
    """the intermediates of the normalising operand: z (+ pb), then (.) sc + sh"""
    t1 = d["R"] + (d["pb"].view(1, -1, 1) if with_pb else 0.0)
    return t1, t1 * d["sc"].unsqueeze(-1) + d["sh"].unsqueeze(-1)


def forward_preconditions(d, acc):
    """[] or the quantities that violate the exactness precondition: a bug in the test's data, never a skip"""
    bias = d["bias"].view(1, -1, 1)
    q = {"acc": acc, "acc + bias": acc + bias, "acc + R": acc + d["R"], "acc + bias + R": acc + bias + d["R"]}
    for with_pb in (False, True):
        t1, t2 = rnorm_terms(d, with_pb)
        tag = "z + pb" if with_pb else "z"
        q.update({tag: t1, f"({tag}) sc + sh": t2, f"acc + ({tag}) sc + sh": acc + t2})
    return [k for k, v in q.items() if not exact_eighths(v)]


# ---- forward ---------------------------------------------------------------------------------------------------------------
def _run_forward_case(case):
    from makani_amd._lib import check, lib, ptr, stream
    dev = torch.device("cuda:0")
    _, B, M, K, N, _ = case
    lda = round8(K)
    d = forward_data(case, dev)
    acc = forward_reference(d)
    assert forward_preconditions(d, acc) == []
    bf, f32 = torch.bfloat16, torch.float32
    wblock = torch.zeros((M, lda), dtype=torch.float64, device=dev)
    wblock[:, :K] = d["w"]
    A, X = operand(wblock, bf), operand(d["x"], bf)
    R, G, bias = operand(d["R"], bf), operand(d["G"], bf), operand(d["bias"], f32)
    Y, P = Guarded((B, M, N), bf, SENT_BF16, dev), Guarded((B, M, N), bf, SENT_BF16, dev)
    b3 = d["bias"].view(1, -1, 1)
    gpos = d["G"] > 0
    fails = []

    def guards(what, outs):
        for name, o in outs:
            if not o.guards_intact():
                fails.append(f"{what}: the guard band around {name} was written")

    for name, (has_b, act, pre, has_r, has_g) in VARIANTS.items():
        what = f"{fwd_id(case)} {name}"
        Y.reset(), P.reset()
        check(lib().mk_conv1x1_nn(ptr(A.t), ptr(X.t), ptr(Y.t), ptr(P.t) if pre else None, ptr(bias.t) if has_b else None,
                                  ptr(R.t) if has_r else None, ptr(G.t) if has_g else None, M, K, lda, B, N, int(act), stream()), what)
        torch.cuda.synchronize()
        guards(what, (("Y", Y), ("Ypre", P)))
        y = Y.t
        lin = acc + b3 if has_b else acc
        if pre:
            fails += describe(what + " pre-activation", mismatch_exact(P.t, lin), P.t, lin)
        elif not bool((P.buf == SENT_BF16).all()):
            fails.append(f"{what}: Ypre was written though none was passed")
        if act and not has_r:
            fails += gelu_gate(what, y, lin)
        elif act:
            # one bf16 step of v is at most 2^-7 |v|: the kernel's GELU is within one step, a kernel that stages the GELU in bf16 adds
            # half a step of it, the final rounding half a step of the sum.  The first premise is gated (gelu_gate) where
            # |gelu| >= 1e-17 only; below that both the kernel's and the exact GELU vanish against any non-zero R and against 1e-16
            gl = gelu_erfc(lin)
            want = gl + d["R"]
            tol = 2.0 ** -7 * (1.5 * gl.abs() + 0.5 * want.abs())
            bad = torch.where(gl.abs() >= 1e-17, mismatch_within(y, want, tol), mismatch_within(y, d["R"], 1e-16))
            fails += describe(what, bad, y, want)
        elif has_g:
            # gelu'(+16) = 1 and gelu'(-16) = 0 to within the 1.5e-7 of the A&S 7.1.26 erf, which saturates at |x| = 16; |acc| < 32,
            # and a relative perturbation of 1e-6 cannot move an exactly representable bf16 value
            r = d["R"] if has_r else torch.zeros_like(acc)
            want = torch.where(gpos, acc + r, r)
            bad = torch.where(gpos, mismatch_exact(y, want), mismatch_within(y, want, 1e-5))
            fails += describe(what, bad, y, want)
        else:
            want = lin + d["R"] if has_r else lin
            fails += describe(what, mismatch_exact(y, want), y, want)

    if lib().mk_conv1x1_nn_rnorm_supported(M, K, lda, B, N):
        coef = operand(torch.stack((d["sc"], d["sh"]), dim=-1).reshape(B * M, 2), f32)
        pb = operand(d["pb"], f32)
        for with_pb in (True, False):
            what = f"{fwd_id(case)} rnorm" + (" + pb" if with_pb else "")
            Y.reset()
            check(lib().mk_conv1x1_nn_rnorm(ptr(A.t), ptr(X.t), ptr(Y.t), None, None, ptr(R.t), None, M, K, lda, B, N, 0, ptr(coef.t),
                                            ptr(pb.t) if with_pb else None, M, stream()), what)
            torch.cuda.synchronize()
            guards(what, (("Y", Y),))
            want = acc + rnorm_terms(d, with_pb)[1]
            fails += describe(what, mismatch_exact(Y.t, want), Y.t, want)
    return fails


def _fwd_param(case):
    return pytest.param(case, id=fwd_id(case))


@pytest.mark.parametrize("case", [_fwd_param(c) for c in FWD_CASES])
def test_forward_exact(case):
    """every epilogue variant of one shape against the one exact expectation; see the module docstring"""
    fails = _run_forward_case(case)
    assert not fails, "\n".join(fails)


# ---- weight gradient --------------------------------------------------------------------------------------------------------
def wgrad_data(case, device):
    _, B, M, K, N = case
    gen = _gen(device, 2000 * M + K + N % 997)
    return {"g": _ints(gen, -3, 3, (B, M, N), device), "x": _ints(gen, -3, 3, (B, K, N), device),
            "preset": _ints(gen, -5, 5, (M, K), device)}


def wgrad_reference(d, chunk=1 << 16):
    B, M, N = d["g"].shape
    dW = torch.zeros((M, d["x"].shape[1]), dtype=torch.float64, device=d["g"].device)
    for b in range(B):
        for n0 in range(0, N, chunk):
            dW += d["g"][b, :, n0:n0 + chunk] @ d["x"][b, :, n0:n0 + chunk].T
    return dW, d["g"].sum(dim=(0, 2))


def wgrad_preconditions(d, dW, db):
    """every sum an integer below 2^24: |g x| <= 9 per term, so the absolute sum bounds every partial sum of every split"""
    bound = float((d["g"].abs().sum(dim=(0, 2)).max()) * 3)
    return bool((dW == dW.round()).all()) and bool((db == db.round()).all()) and bound < 2.0 ** 24


def _run_wgrad_case(case):
    from makani_amd._lib import check, lib, ptr, stream
    dev = torch.device("cuda:0")
    _, B, M, K, N = case
    d = wgrad_data(case, dev)
    dW_ref, db_ref = wgrad_reference(d)
    assert wgrad_preconditions(d, dW_ref, db_ref)
    G, X = operand(d["g"], torch.bfloat16), operand(d["x"], torch.bfloat16)
    f32 = torch.float32
    nws = lib().mk_conv1x1_wgrad_workspace(M, K, B, N)
    dW, db, part = Guarded((M, K), f32, SENT_F32, dev), Guarded((M,), f32, SENT_F32, dev), Guarded((nws,), f32, SENT_F32, dev)
    fused = bool(lib().mk_conv1x1_wgrad_fuses_bias(M, K, B, N))
    fails = []
    runs = [("wgrad", False, 0)] + ([("wgrad + bias gradient", True, 0)] if fused else [])
    if case in WG_ACCUMULATE:
        runs += [("wgrad accumulate", False, 1)] + ([("wgrad + bias gradient accumulate", True, 1)] if fused else [])
    for name, with_db, accumulate in runs:
        what = f"{wg_id(case)} {name}"
        dW.reset(), db.reset(), part.reset()
        if accumulate:
            dW.t.copy_(d["preset"])
        if with_db:
            check(lib().mk_conv1x1_wgrad_bias(ptr(G.t), ptr(X.t), ptr(dW.t), ptr(db.t), ptr(part.t), M, K, B, N, accumulate, stream()), what)
        else:
            check(lib().mk_conv1x1_wgrad(ptr(G.t), ptr(X.t), ptr(dW.t), ptr(part.t), M, K, B, N, accumulate, stream()), what)
        torch.cuda.synchronize()
        for nm, o in (("dW", dW), ("db", db), ("the split workspace", part)):
            if not o.guards_intact():
                fails.append(f"{what}: the guard band around {nm} was written")
        want = dW_ref + d["preset"] if accumulate else dW_ref
        fails += describe(what + " dW as (0, m, k)", mismatch_exact(dW.t, want).unsqueeze(0), dW.t.unsqueeze(0), want.unsqueeze(0))
        if with_db:
            # include/makani_amd.h: db is OVERWRITTEN whatever `accumulate` says (the launcher hands the bias reducer 0); it held
            # the sentinel before the call
            fails += describe(what + " db as (0, 0, m)", mismatch_exact(db.t, db_ref).view(1, 1, -1), db.t.view(1, 1, -1), db_ref.view(1, 1, -1))
        elif not bool((db.buf == SENT_F32).all()):
            fails.append(f"{what}: db was written though none was passed")
    return fails


@pytest.mark.parametrize("case", [pytest.param(c, id=wg_id(c)) for c in WG_CASES])
def test_wgrad_exact(case):
    """dW = sum g x and db = sum g exactly in fp32, with and without the fused bias gradient and with accumulate = 1"""
    fails = _run_wgrad_case(case)
    assert not fails, "\n".join(fails)


# ---- the process-wide switches ----------------------------------------------------------------------------------------------
# measured on the MI355X: 7.0 - 7.8 s per child (a fresh interpreter: most of it is start-up, the matrix itself runs 3 s);
# the margin is for a box that other work shares (docs/LAB_NOTEBOOK.md)
CHILD_TIMEOUT = 60


@pytest.mark.parametrize("env", [{"MAKANI_AMD_ASTAT2": "0", "MAKANI_AMD_CONV_NT": "0", "MAKANI_AMD_RING384": "0"},
                                 {"MAKANI_AMD_ASTAT2": "1", "MAKANI_AMD_CONV_NT": "1"}], ids=["astat1-st-ring192", "astat2-nt"])
def test_forward_exact_under_the_switches(env):
    """MAKANI_AMD_ASTAT2, MAKANI_AMD_CONV_NT and MAKANI_AMD_RING384 are read once per process and the expected values do not
    depend on them: the forward matrix without the long-stream cases in two fresh child processes (the one-group stationary
    kernel, default stores, never the 384-row tile; the two-group kernel also at shard sizes, streaming stores)"""
    torch.cuda.synchronize()                        # a child is started from a healthy device only
    out =subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_conv_exact.py"), "-q", "-x", "-m", "gpu",
                          "-k", "test_forward_exact and not switches and not longstream"], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-4000:] + out.stderr[-1000:]
