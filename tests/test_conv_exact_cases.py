"""The case tables of tests/test_gpu_conv_exact.py against the plan itself, on the CPU: csrc/conv1x1_plan.h (conv_nn_plan,
conv_nn_ring_rows, conv_nn_rnorm_supported, wgrad_plan: plain C++) is compiled for the host as tests/test_conv_ring_plan.py does,
and the tables must reach every kernel, template variant, tile height and reducer.  A case edited so that a branch is no longer
reached fails here, without a GPU.  Also the unit test of the comparison helpers: one wrong element, or one 16-byte vector left
at the sentinel, is reported with its (b, m, n)."""
import ctypes
import subprocess

import pytest
import torch

import test_gpu_conv_exact as gx

ASTAT73, ASTAT2, ASTAT1, RING, TILE = range(5)          # enum class ConvNnKernel, in the order of its declaration
NAMES = {ASTAT73: "astat73", ASTAT2: "astat2", ASTAT1: "astat1", RING: "ring", TILE: "tile"}

SHIM = r"""
#include "conv1x1_plan.h"
static_assert((int)ConvNnKernel::astat73 == 0 && (int)ConvNnKernel::astat2 == 1 && (int)ConvNnKernel::astat1 == 2 &&
              (int)ConvNnKernel::ring == 3 && (int)ConvNnKernel::tile == 4, "the Python side numbers the kernels in this order");
extern "C" int plan(int M, int K, int lda, int B, long long N, int pre, int r, int g, int env) {
    return (int)conv_nn_plan(M, K, lda, B, N, pre != 0, r != 0, g != 0, env);
}
extern "C" int rows(int M, int K, int B, long long N, int epi, int env) { return conv_nn_ring_rows(M, K, B, N, epi != 0, env); }
extern "C" int rnorm(int M, int K, int lda, int B, long long N, int env) { return conv_nn_rnorm_supported(M, K, lda, B, N, env) ? 1 : 0; }
extern "C" void wplan(int M, int K, int B, long long N, long long* out) {
    const WgPlan pl = wgrad_plan(M, K, B, N);
    out[0] = pl.ring, out[1] = pl.swap, out[2] = pl.tp, out[3] = pl.slabs, out[4] = pl.qslabs, out[5] = pl.S, out[6] = pl.chunk;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from makani_amd import build
    d = tmp_path_factory.mktemp("conv_exact_plan")
    src = d / "plan.cpp"
    src.write_text(SHIM)
    so = str(d / "plan.so")
    subprocess.check_call([build.HIPCC, "-x", "c++", "-std=c++17", "-shared", "-fPIC", "-I", build.CSRC, str(src), "-o", so])
    L = ctypes.CDLL(so)
    ll, i = ctypes.c_longlong, ctypes.c_int
    L.plan.argtypes = [i, i, i, i, ll, i, i, i, i]
    L.rows.argtypes = [i, i, i, ll, i, i]
    L.rnorm.argtypes = [i, i, i, i, ll, i]
    L.wplan.argtypes = [i, i, i, ll, ctypes.POINTER(ll)]
    L.wplan.restype = None
    return L


def launches(L, case, astat2_env=-1, ring384_env=-1):
    """what mk_conv1x1_nn launches for every variant of a forward case: {variant: (kernel, PRE, EPI_LOADS, tile height or width,
    tiles the least loaded workgroup walks, ring slots)} from the plan and the grid formulas of the launcher (csrc/conv1x1.hip)"""
    _, B, M, K, N, _ = case
    lda = gx.round8(K)
    out = {}
    for name, (_, act, stored, has_r, has_g) in gx.VARIANTS.items():
        pre, epi = bool(act and stored), bool(has_r or has_g)
        k = L.plan(M, K, lda, B, N, pre, has_r, has_g, astat2_env)
        slabs, tn64 = (M + 383) // 384, (N + 63) // 64
        if k in (ASTAT73, ASTAT2, ASTAT1):
            wgs = (256 if epi else 512) if k == ASTAT73 else 256            # stationary_grid
            streams = min(tn64, wgs // slabs)
            # ring slots: conv_nn_astat_kernel NSLOT (one chunk per tile with K <= 80), conv_nn_astat2_kernel NSLOT
            slots = (8 if epi else 5) if k == ASTAT73 else 4
            out[name] = (k, pre, epi, 384, tn64 // streams, slots)
        elif k == RING:
            bm = L.rows(M, K, B, N, bool(act or stored or has_r or has_g), ring384_env)
            nt = ((M + bm - 1) // bm) * ((N + 255) // 256) * B
            out[name] = (k, False, False, bm, nt // min(nt, 256), 2)       # a two-stage ring
        else:
            out[name] = (k, False, False, 256 if N >= 1 << 19 else 128, 1, 0)
    return out


def test_every_forward_case_runs_the_kernel_it_is_listed_under(plan):
    for case in gx.FWD_CASES:
        assert NAMES[launches(plan, case)["plain"][0]] == case[0], case


def test_the_forward_table_reaches_every_kernel_form(plan):
    hit = set()
    for case in gx.FWD_CASES:
        hit |= {v[:4] for v in launches(plan, case).values()}
    both = [(p, e) for p in (False, True) for e in (False, True)]
    # the 73-channel kernel hands pre-activation AND operand to the ring kernel: three forms
    assert {(p, e) for k, p, e, _ in hit if k == ASTAT73} == {(False, False), (True, False), (False, True)}
    assert {(p, e) for k, p, e, _ in hit if k == ASTAT2} == set(both)
    assert not any(k == ASTAT1 for k, *_ in hit)                            # MAKANI_AMD_ASTAT2=0 only
    assert {h for k, _, _, h in hit if k == RING} == {192, 256, 384}
    assert {h for k, _, _, h in hit if k == TILE} == {128, 256}
    # ... and the one-group kernel under MAKANI_AMD_ASTAT2=0, the first child process of the switch test
    hit0 = set()
    for case in gx.FWD_CASES:
        if not case[5]:
            hit0 |= {v[:3] for v in launches(plan, case, astat2_env=0, ring384_env=0).values()}
    assert {(p, e) for k, p, e in hit0 if k == ASTAT1} == set(both)
    assert not any(k == ASTAT2 for k, *_ in hit0)


def test_the_cases_named_for_a_dispatch_branch_take_it(plan):
    by = {c[1:5]: launches(plan, c) for c in gx.FWD_CASES}
    # pre-activation and an operand together leave the 73-channel kernel for the ring kernel (ragged second k-tile: K = 73)
    assert by[(1, 256, 73, 264)]["bias_gelu_pre_res"][0] == RING and by[(1, 256, 73, 264)]["res"][0] == ASTAT73
    # both operands together leave the stationary kernels
    assert by[(1, 768, 384, 328)]["dgelu_res"][0] == RING and by[(1, 768, 384, 328)]["dgelu"][0] == ASTAT2
    # the two sides of small_ring (B N = 32 768): at it the ring kernel, but for a stored pre-activation
    at, above = by[(1, 384, 384, 32768)], by[(1, 384, 384, 32776)]
    assert {n for n, v in at.items() if v[0] == ASTAT2} == {"bias_gelu_pre", "bias_gelu_pre_res"}
    assert all(v[0] == RING for n, v in at.items() if "pre" not in n)
    assert all(v[0] == ASTAT2 for n, v in above.items() if n != "dgelu_res")
    # one k-tile on the ring kernel; the 384-row tile for plain and + bias only, with a workgroup that takes two tiles
    assert by[(1, 192, 64, 256)]["plain"][:4] == (RING, False, False, 192)
    wide = by[(1, 384, 768, 65544)]
    assert {n for n, v in wide.items() if v[3] == 384} == {"plain", "bias"} and all(v[3] == 192 for n, v in wide.items() if n not in ("plain", "bias"))
    assert ((65544 + 255) // 256) == 257
    # N < 64 keeps K = 384 off the stationary kernels
    assert all(v[0] == TILE for v in by[(1, 300, 384, 56)].values())


def test_the_normalising_operand_is_served_for_at_least_three_cases(plan):
    served = [c for c in gx.FWD_CASES if plan.rnorm(c[2], c[3], gx.round8(c[3]), c[1], c[4], -1)]
    assert len(served) >= 3, served


def test_long_stream_cases_give_a_workgroup_more_tiles_than_the_ring_has_slots(plan):
    long_cases = [c for c in gx.FWD_CASES if c[5]]
    assert {c[0] for c in long_cases} == {"astat73", "astat2", "ring"}
    for case in long_cases:
        for name, (k, _, _, _, tiles, slots) in launches(plan, case).items():
            assert k != TILE and tiles > slots, (case, name, NAMES[k], tiles, slots)


def wplan(L, case):
    _, B, M, K, N = case
    out = (ctypes.c_longlong * 7)()
    L.wplan(M, K, B, N, out)
    return dict(zip(("ring", "swap", "tp", "slabs", "qslabs", "S", "chunk"), out))


def test_the_weight_gradient_table_reaches_every_plan(plan):
    plans = {c: wplan(plan, c) for c in gx.WG_CASES}
    for c, pl in plans.items():
        assert ("ring" if pl["ring"] else "tile") == c[0], (c, pl)
    ring = [pl for pl in plans.values() if pl["ring"]]
    # both slab heights with either operand as P, and one and two 384-row slabs of Q with either operand as Q
    assert {(pl["tp"], pl["swap"]) for pl in ring} == {(192, 0), (192, 1), (256, 0), (256, 1)}
    assert {(pl["qslabs"], pl["swap"]) for pl in ring} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert any(pl["slabs"] > 1 and pl["tp"] == 192 for pl in ring) and any(pl["slabs"] > 1 and pl["tp"] == 256 for pl in ring)
    assert any(not pl["ring"] for pl in plans.values())
    # reduce_splits4 (M K a multiple of 4; the test's buffers are 16-byte aligned) and the scalar reduce_splits, each with splits
    vec = {c: c[2] * c[3] % 4 == 0 for c in plans}
    assert any(v and plans[c]["S"] > 1 for c, v in vec.items()) and any(not v and plans[c]["S"] > 1 for c, v in vec.items())
    assert plans[("tile", 1, 64, 64, 4104)]["S"] == 3 and plans[("ring", 2, 384, 384, 8200)]["S"] == 34
    assert any(pl["S"] >= 8 and pl["S"] % 8 for pl in plans.values())      # both loops of a reducer
    # accumulate = 1: a tile-kernel case on reduce_splits4 and a ring-kernel case on the scalar form
    acc = {c: plans[c] for c in gx.WG_ACCUMULATE}
    assert {(bool(pl["ring"]), vec[c]) for c, pl in acc.items()} == {(False, True), (True, False)}


# ---- the test's own data and helpers --------------------------------------------------------------------------------------------
SMALL = [c for c in gx.FWD_CASES if c[1] * c[2] * c[4] <= 300000]


@pytest.mark.parametrize("case", [pytest.param(c, id=gx.fwd_id(c)) for c in SMALL])
def test_the_forward_data_meets_the_exactness_precondition(case):
    """the small cases on the CPU (the GPU test asserts it for every case before it runs a kernel)"""
    d = gx.forward_data(case, torch.device("cpu"))
    acc = gx.forward_reference(d)
    assert gx.forward_preconditions(d, acc) == []
    assert torch.equal(d["w"].float() @ d["x"][0].float(), acc[0].float())          # fp32 and fp64 products are identical
    assert torch.equal((acc + d["bias"].view(1, -1, 1)).bfloat16().double(), acc + d["bias"].view(1, -1, 1))
    d["R"][0, 0, 0] = 40.0                                                            # out of range: the precondition names it
    assert "acc + R" in gx.forward_preconditions(d, acc)


def test_a_weight_gradient_case_meets_its_precondition():
    case = ("tile", 2, 129, 130, 136)
    d = gx.wgrad_data(case, torch.device("cpu"))
    dW, db = gx.wgrad_reference(d)
    assert gx.wgrad_preconditions(d, dW, db)
    assert torch.equal(torch.einsum("bmn,bkn->mk", d["g"].float(), d["x"].float()).double(), dW)


def test_the_comparison_reports_one_wrong_element_and_one_unwritten_vector():
    case = ("tile", 2, 129, 72, 136, False)
    d = gx.forward_data(case, torch.device("cpu"))
    want = gx.forward_reference(d) + d["bias"].view(1, -1, 1)
    good = want.bfloat16()
    assert gx.describe("ok", gx.mismatch_exact(good, want), good, want) == []
    neg0 = good.clone()
    neg0[want == 0] = -0.0                                                            # -0 = +0
    assert int((want == 0).sum()) > 0 and not bool(gx.mismatch_exact(neg0, want).any())
    # one element off by one bf16 step of its neighbourhood (1/8)
    y = good.clone()
    y[1, 128, 135] += 0.125
    count, first = gx.first_mismatches(gx.mismatch_exact(y, want), y, want)
    assert count == 1 and first[0][:3] == (1, 128, 135) and first[0][3] == first[0][4] + 0.125
    assert "(1, 128, 135)" in gx.describe("flip", gx.mismatch_exact(y, want), y, want)[0]
    # one 16-byte vector (8 pixels) left at the sentinel
    y = good.clone()
    y[0, 77, 128:136] = gx.SENT_BF16
    count, first = gx.first_mismatches(gx.mismatch_exact(y, want), y, want)
    assert count == 8 and [f[:3] for f in first] == [(0, 77, n) for n in range(128, 136)] and first[0][3] == gx.SENT_BF16
    # a NaN that an operand's surroundings let in
    y = good.clone()
    y[0, 0, 0] = float("nan")
    assert gx.first_mismatches(gx.mismatch_exact(y, want), y, want)[1][0][:3] == (0, 0, 0)
    assert gx.first_mismatches(gx.mismatch_within(y, want, 1e-5), y, want)[1][0][:3] == (0, 0, 0)


def test_the_gelu_gate_sees_a_second_step_and_an_unwritten_tail():
    pre = torch.arange(-80, 81, dtype=torch.float64).div(8).repeat(1, 4, 8)          # -10 ... 10 in eighths: includes 0 and the tail
    want = gx.gelu_erfc(pre).bfloat16()
    assert gx.gelu_gate("ok", want, pre) == []
    i = int((pre[0, 0] == 1.0).nonzero()[0])
    y = want.clone()
    y.view(torch.int16)[0, 2, i] += 1                                                 # one step: inside the gate (and 99.9 % still identical)
    assert gx.gelu_gate("one", y, pre) == []
    y.view(torch.int16)[0, 2, i] += 1
    assert "(0, 2, %d)" % i in gx.gelu_gate("two", y, pre)[0]
    y = want.clone()
    y[0, 3, 0] = gx.SENT_BF16                                                         # pre = -10: below 1e-17, where no step count applies
    assert "(0, 3, 0)" in gx.gelu_gate("tail", y, pre)[0]


def test_a_guarded_buffer_notices_a_write_behind_its_slice():
    g = gx.Guarded((3, 5), torch.float32, gx.SENT_F32, torch.device("cpu"))
    assert g.g * 4 == gx.GUARD_BYTES and g.buf.numel() == 15 + 2 * g.g and g.guards_intact()
    g.t.fill_(1.0)
    assert g.guards_intact()
    g.buf[g.g + 15] = 0.0
    assert not g.guards_intact()
    g.reset()
    assert g.guards_intact() and bool((g.t == gx.SENT_F32).all())
    o = gx.operand(torch.ones(2, 8), torch.bfloat16)
    assert bool(o.buf[:o.g].isnan().all()) and bool(o.buf[o.g + 16:].isnan().all()) and bool((o.t == 1).all())
