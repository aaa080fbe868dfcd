"""The output constraints (csrc/constraints.hip behind ``makani_amd.constraints``) on the GPU against the fp64 restatement
tests/_constraints_ref.py, itself pinned against the reference's classes by tests/test_constraints.py.

Gates.  f32: 2 x the reference's own fp32 error + one fp32 ulp of the largest magnitude of the compared tensor.  For a fixture
case the reference's error is the recorded ``err32_out`` / ``err32_grad`` (the class's own fp32 CPU run against its double run);
for inputs generated here it is the distance between the restated formula in fp32 torch and in fp64 on those very inputs.  The
factor 2: another summation order and FMA contraction over at most 2 L + 1 terms have the error bound of the reference's own
order.  bf16: the result equals the fp64 restatement of the bf16 inputs, rounded to bf16, or is its neighbour.  Neither gate
is taken from the code under test."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _constraints_ref as ref          # noqa: E402
from conftest import load_golden          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ref.load_cases(load_golden("constraints.npz"))
NAMES = sorted(CASES)
LAYERS = ["wrapper_moist", "projection_moist_s07_clim", "nonneg_softplus"]          # one of each kind, the richest form


def ulp32(t):
    m = float(t.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 0.0


def build(case, **override):
    import makani_amd.constraints as mc
    c = CASES[case]
    m = c["meta"]
    kw = dict(m["kwargs"])
    if m["kind"] == "projection":
        kw["climatology_offset"] = c["climatology_offset"] if kw["climatology_offset"] else None
    kw.update(override)
    cls = {"wrapper": mc._HydrostaticBalanceWrapper, "projection": mc.HydrostaticBalanceProjection, "nonneg": mc.NonNegativeConstraint}[m["kind"]]
    return cls(channel_names=m["channel_names"], bias=c.get("bias"), scale=c.get("scale"), **kw).train(m["training"]).to(DEV)


def run(mod, x, g):
    """output and input gradient of the module under test"""
    x = x.detach().requires_grad_(True)
    y = mod(x)
    (gx,) = torch.autograd.grad(y, x, g)
    return y.detach(), gx


def quantised(shape, gen):
    return torch.clamp(torch.round(32.0 * torch.randn(*shape, generator=gen)), -127, 127) / 32.0


def bf16_steps(a, b):
    """distance of two bf16 tensors in representable values"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs().max().item()


@pytest.mark.parametrize("case", NAMES)
def test_f32_parity_with_the_restatement(case):
    c = CASES[case]
    kind = c["meta"]["kind"]
    want_y, want_g = ref.FWD[kind](c["x"], c["buf"], c["meta"]), ref.BWD[kind](c["x"], c["g"], c["buf"], c["meta"])
    y, gx = run(build(case), c["x"].to(DEV), c["g"].to(DEV))
    assert y.dtype == torch.float32 and y.shape == want_y.shape and gx.shape == want_g.shape
    e_out, e_grad = (y.cpu().double() - want_y).abs().max().item(), (gx.cpu().double() - want_g).abs().max().item()
    gate_out, gate_grad = 2.0 * float(c["err32_out"]) + ulp32(want_y), 2.0 * float(c["err32_grad"]) + ulp32(want_g)
    print(f"{case}: out {e_out:.3e} (gate {gate_out:.3e})  grad {e_grad:.3e} (gate {gate_grad:.3e})")
    assert e_out <= gate_out and e_grad <= gate_grad


@pytest.mark.parametrize("case", NAMES)
def test_bf16_parity_with_the_restatement(case):
    """bf16 inputs (the fixture's, which bf16 holds exactly): the result is the fp64 restatement rounded to bf16, or its neighbour.

    ``projection_dry_s07`` is the case that tells the evaluations apart: one of its 840 projected values is 2.083e-05, where a
    bf16 step is 1.2e-07, next to a state of O(10).  The formula taken step by step in fp32 carries an absolute error of about
    3e-07 there (the reference's own fp32 run is 4 steps off, well inside the f32 gate), so the dry forward sums the folded
    affine map with error compensation and rounds once."""
    c = CASES[case]
    kind = c["meta"]["kind"]
    xb, gb = c["x"].bfloat16(), c["g"].bfloat16()
    want_y = ref.FWD[kind](xb.double(), c["buf"], c["meta"]).bfloat16()
    want_g = ref.BWD[kind](xb.double(), gb.double(), c["buf"], c["meta"]).bfloat16()
    y, gx = run(build(case), xb.to(DEV), gb.to(DEV))
    assert y.dtype == torch.bfloat16 and gx.dtype == torch.bfloat16
    s_out, s_grad = bf16_steps(y.cpu(), want_y), bf16_steps(gx.cpu(), want_g)
    j = int((y.cpu().float() - want_y.float()).abs().argmax())
    print(f"{case}: bf16 steps out {s_out} grad {s_grad}; largest output difference at {want_y.flatten()[j].item():.6e} "
          f"(got {y.cpu().flatten()[j].item():.6e})")
    assert s_out <= 1 and s_grad <= 1


def _generated(case, shape, seed, mod=None):
    """a layer of a fixture case on an input of another shape: (module, x, g, want_y, want_g, gate_out, gate_grad); the buffers
    of the restatement are the module's own (pinned to the reference's by tests/test_constraints.py)"""
    c = CASES[case]
    kind, meta = c["meta"]["kind"], c["meta"]
    mod = build(case) if mod is None else mod
    buf = {k: v.detach().cpu() for k, v in mod.named_buffers()}
    gen = torch.Generator().manual_seed(seed)
    Bn, H, W = shape
    c_in = meta["N_in_channels"] if kind == "wrapper" else len(meta["channel_names"])
    x, g = quantised((Bn, c_in, H, W), gen), quantised((Bn, len(meta["channel_names"]), H, W), gen)
    want_y, want_g = ref.FWD[kind](x, buf, meta), ref.BWD[kind](x, g, buf, meta)
    y32, g32 = ref.FWD[kind](x, buf, meta, dtype=torch.float32), ref.BWD[kind](x, g, buf, meta, dtype=torch.float32)
    gate_out = 2.0 * (y32.double() - want_y).abs().max().item() + ulp32(want_y)
    gate_grad = 2.0 * (g32.double() - want_g).abs().max().item() + ulp32(want_g)
    return mod, x, g, want_y, want_g, gate_out, gate_grad


def _check(mod, xd, gd, want_y, want_g, gate_out, gate_grad, what):
    y, gx = run(mod, xd, gd)
    e_out, e_grad = (y.cpu().double() - want_y).abs().max().item(), (gx.cpu().double() - want_g).abs().max().item()
    print(f"{what}: out {e_out:.3e} (gate {gate_out:.3e})  grad {e_grad:.3e} (gate {gate_grad:.3e})")
    assert e_out <= gate_out and e_grad <= gate_grad
    return y, gx


# W = 7: the scalar path; W = 16: the 16-byte path; 3 x 1030: HW = 3090 = 2 mod 4 (scalar, 13 blocks per plane, the last one short);
# 4 x 1030: HW = 4120 (16-byte path, 5 blocks per plane, the last one short)
SHAPES = [(1, 5, 7), (3, 3, 16), (1, 3, 1030), (3, 4, 1030)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", LAYERS + ["wrapper_dry", "projection_dry_s10_clim", "wrapper_two_levels", "projection_two_levels"])
def test_shapes_beyond_the_fixture(case, shape):
    mod, x, g, want_y, want_g, go, gg = _generated(case, shape, 11 + shape[2])
    _check(mod, x.to(DEV), g.to(DEV), want_y, want_g, go, gg, f"{case} {shape}")


@pytest.mark.parametrize("case", ["wrapper_dry", "projection_dry_s07", "projection_window_of_13"])
def test_dry_forward_in_bf16_next_to_zero(case):
    """The bf16 gate over 1.5e5 to 3.6e5 outputs per case (the generated inputs are multiples of 1 / 32, which bf16 holds exactly): among so
    many, outputs a thousand times smaller than the state occur by chance, and there a sum taken step by step in fp32 is several
    bf16 steps off.  The dry forward is the fp64 value rounded once, so it is within one step at every magnitude."""
    mod, x, _, want_y, _, _, _ = _generated(case, (3, 4, 1030), 23)
    with torch.no_grad():
        y = mod(x.bfloat16().to(DEV))
    steps = bf16_steps(y.cpu(), want_y.bfloat16())
    print(f"{case}: bf16 steps {steps} over {want_y.numel()} outputs, {int((want_y.abs() < 1e-2).sum())} of them below 1e-2, "
          f"smallest non-zero {want_y[want_y != 0].abs().min().item():.3e}")
    assert y.dtype == torch.bfloat16 and steps <= 1


@pytest.mark.parametrize("case", LAYERS)
def test_misaligned_and_non_contiguous_inputs(case):
    mod, x, g, want_y, want_g, go, gg = _generated(case, (2, 3, 16), 5)
    # a contiguous view whose storage starts one element off a 16-byte boundary: the scalar path
    flat = torch.empty(x.numel() + 1, device=DEV)
    off = flat[1:].view(x.shape)
    off.copy_(x)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    y0, g0 = _check(mod, off, g.to(DEV), want_y, want_g, go, gg, f"{case} misaligned")
    # channels-last and a transposed grid: made contiguous, not rejected
    xd = x.to(DEV)
    y1, g1 = _check(mod, xd.contiguous(memory_format=torch.channels_last), g.to(DEV), want_y, want_g, go, gg, f"{case} channels_last")
    xt = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not xt.is_contiguous()
    y2, g2 = _check(mod, xt, g.to(DEV).transpose(-1, -2).contiguous().transpose(-1, -2), want_y, want_g, go, gg, f"{case} transposed")
    ya, ga = run(mod, xd, g.to(DEV))          # the aligned 16-byte path: the same arithmetic per pixel
    for y, gx in ((y0, g0), (y1, g1), (y2, g2)):
        assert torch.equal(y, ya) and torch.equal(gx, ga)


def _sixteen_levels(moist):
    levels = [1000, 925, 850, 775, 700, 600, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30]
    names = ["u10m"] + [f"{v}{p}" for p in levels[::-1] for v in ("t", "q", "z")] + ["sp"]
    gen = torch.Generator().manual_seed(3)
    bias, scale = [], []
    for n in names:
        k = math.log(1000.0 / int(n[1:])) / math.log(20.0) if n[0] in "tqz" and n[1:].isdigit() else 0.0
        b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3 * (0.8 + 0.4 * k)), "t": (285.0 - 70.0 * k, 15.0 - 4.0 * k), "q": (2.0e-3, 2.0e-3),
                "u": (0.5, 5.0), "s": (9.7e4, 9.0e3)}[n[0]]
        bias.append(b)
        scale.append(s * (0.9 + 0.2 * float(torch.rand(1, generator=gen))))
    return names, torch.tensor(bias).view(1, -1, 1, 1), torch.tensor(scale).view(1, -1, 1, 1)


@pytest.mark.parametrize("kind", ["wrapper", "projection"])
@pytest.mark.parametrize("moist", [False, True])
def test_sixteen_levels(kind, moist):
    import makani_amd.constraints as mc
    names, bias, scale = _sixteen_levels(moist)
    if kind == "wrapper":
        mod = mc._HydrostaticBalanceWrapper(names, bias, scale, p_min=0, p_max=2000, use_moist_air_formula=moist).to(DEV)
        meta = dict(kind=kind, channel_names=names, z_idx=mod.z_idx, t_idx=mod.t_idx, moist=moist, N_in_channels=mod.mapping.shape[1],
                    q_idx=mod.q_idx if moist else None)
    else:
        mod = mc.HydrostaticBalanceProjection(names, bias, scale, p_min=0, p_max=2000, strength=0.9, use_moist_air_formula=moist,
                                              climatology_offset=torch.linspace(-30.0, 30.0, 15)).to(DEV)
        meta = dict(kind=kind, channel_names=names, channel_indices=mod.channel_indices.tolist(), num_levels=16, strength=0.9, moist=moist,
                    q_indices=mod.q_indices.tolist() if moist else None)
    assert len(meta.get("z_idx", range(16))) == 16
    CASES["_sixteen"] = {"meta": meta}
    try:
        for shape in ((2, 5, 7), (1, 3, 16)):
            _, x, g, want_y, want_g, go, gg = _generated("_sixteen", shape, 21, mod=mod)
            _check(mod, x.to(DEV), g.to(DEV), want_y, want_g, go, gg, f"16 levels {kind} moist={moist} {shape}")
    finally:
        del CASES["_sixteen"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["wrapper_moist", "wrapper_window_of_13", "projection_moist_s10", "projection_window_of_13", "nonneg_silu",
                                  "nonneg_eval"])
def test_untouched_channels_are_bit_identical_copies(case, dtype):
    c = CASES[case]
    m = c["meta"]
    for shape in ((2, 5, 7), (2, 3, 16)):
        gen = torch.Generator().manual_seed(9)
        c_in = m["N_in_channels"] if m["kind"] == "wrapper" else len(m["channel_names"])
        x = torch.randn(shape[0], c_in, *shape[1:], generator=gen).to(dtype).to(DEV)
        g = torch.randn(shape[0], len(m["channel_names"]), *shape[1:], generator=gen).to(dtype).to(DEV)
        y, gx = run(build(case), x, g)
        if m["kind"] == "wrapper":
            dst = m["aux_idx"]
            src = list(range(c_in - len(dst), c_in))
        else:
            touched = set(m["channel_indices"])
            dst = src = [i for i in range(c_in) if i not in touched and i not in (m.get("q_indices") or [])]
        assert len(dst) >= 2
        assert torch.equal(y[:, dst], x[:, src]) and torch.equal(gx[:, src], g[:, dst])


# ---- physics ----------------------------------------------------------------------------------------------------------------
def test_wrapper_returns_the_profile_its_geopotentials_were_integrated_from():
    """the reference's test_hydrostatic_balance_matches_independent_integration at (2, 3, 4): hypsometric geopotentials of a
    known temperature profile, integrated here level by level in fp64, give that profile back"""
    import makani_amd.constraints as mc
    c = CASES["wrapper_window_of_13"]
    m = c["meta"]
    mod = build("wrapper_window_of_13")
    p, L = m["pressures"], len(m["pressures"])
    gen = torch.Generator().manual_seed(4)
    T = 288.0 - 6.0 * torch.arange(L, dtype=torch.float64).view(1, L, 1, 1) + 3.0 * torch.rand(2, L, 3, 4, generator=gen).double()
    Z = torch.zeros_like(T)
    Z[:, 0] = 1.5e4 + 100.0 * torch.rand(2, 3, 4, generator=gen).double()
    for i in range(1, L):
        Z[:, i] = Z[:, i - 1] + 0.5 * ref.R_DRY * math.log(p[i - 1] / p[i]) * (T[:, i] + T[:, i - 1])
    bias, scale = c["bias"].double(), c["scale"].double()
    x = torch.zeros(2, m["N_in_channels"], 3, 4, dtype=torch.float64)
    x[:, 0] = (T[:, 0] - bias[0, m["t_idx"][0], 0, 0]) / scale[0, m["t_idx"][0], 0, 0]
    x[:, 1: L + 1] = (Z - bias[:, m["z_idx"]]) / scale[:, m["z_idx"]]
    x32 = x.float()
    want = ref.wrapper_fwd(x32, c["buf"], m)
    err32 = (ref.wrapper_fwd(x32, c["buf"], m, dtype=torch.float32).double() - want).abs().max().item()
    y = mod(x32.to(DEV)).cpu().double()
    assert (y - want).abs().max().item() <= 2.0 * err32 + ulp32(want)
    # and the profile itself, up to what rounding x to fp32 moves it by (the restatement of the rounded input measures that)
    T_got = y[:, m["t_idx"]] * scale[:, m["t_idx"]] + bias[:, m["t_idx"]]
    T_want = want[:, m["t_idx"]] * scale[:, m["t_idx"]] + bias[:, m["t_idx"]]
    moved = (T_want - T).abs().max().item()
    print(f"profile: |T_got - T| {(T_got - T).abs().max().item():.3e}, of which input rounding {moved:.3e}")
    assert (T_got - T).abs().max().item() <= moved + (2.0 * err32 + ulp32(want)) * float(scale[:, m["t_idx"]].max())


def _constraint_matrix(pressures):
    L = len(pressures)
    A = torch.zeros(L - 1, 2 * L, dtype=torch.float64)
    for i in range(1, L):
        ci = 0.5 * ref.R_DRY * math.log(pressures[i - 1] / pressures[i])
        A[i - 1, L + i], A[i - 1, L + i - 1], A[i - 1, i], A[i - 1, i - 1] = 1.0, -1.0, -ci, -ci
    return A


@pytest.mark.parametrize("case", ["projection_dry_s10_clim", "projection_moist_s10_clim", "projection_window_of_13"])
def test_projected_state_satisfies_the_balance_relation(case):
    import makani_amd.constraints as mc
    c = CASES[case]
    m = c["meta"]
    L, idx = m["num_levels"], m["channel_indices"]
    names = m["channel_names"]
    pressures = mc.get_matching_channels_pl(names, "z", "t", m["kwargs"]["p_min"], m["kwargs"]["p_max"])[2]
    all_p = mc.get_matching_channels_pl(names, "z", "t", float("-inf"), float("inf"))[2]
    start = all_p.index(pressures[0])
    b_clim = c["climatology_offset"].double()[start: start + L - 1]
    A = _constraint_matrix(pressures)
    y = build(case)(c["x"].to(DEV)).cpu().double()

    def residual(out):
        phys = out[:, idx] * c["buf"]["scale_sub"].double() + c["buf"]["bias_sub"].double()
        if m["moist"]:
            q = out[:, m["q_indices"]] * c["buf"]["q_scale"].double() + c["buf"]["q_bias"].double()
            phys = torch.cat([phys[:, :L] * (1.0 + ref.Q_EPS * q), phys[:, L:]], dim=1)
        return torch.einsum("rc,bchw->brhw", A, phys) - b_clim.view(1, -1, 1, 1)

    # the same gate as the parity test, carried into the residual: |A| (gate * scale), row by row
    gate = 2.0 * float(c["err32_out"]) + ulp32(c["out"])
    bound = (A.abs() @ (gate * c["buf"]["scale_sub"].double().reshape(-1))).max().item() * (1.0 + ref.Q_EPS * 0.02)
    floor = residual(c["out"]).abs().max().item()          # what the fp32 operator of the reference leaves in exact arithmetic
    got = residual(y).abs().max().item()
    print(f"{case}: residual {got:.3e} m2/s2 (fp64 evaluation of the recorded operator {floor:.3e}, bound {bound:.3e})")
    assert got <= floor + bound
    before = residual(c["x"].double()).abs().max().item()
    assert got < 1e-3 * before


@pytest.mark.parametrize("strength", [1.0, 0.3])
@pytest.mark.parametrize("case", ["projection_dry_s10_clim", "projection_moist_s10_clim"])
def test_a_balanced_state_is_unchanged_at_any_strength(case, strength):
    c = CASES[case]
    m = c["meta"]
    idx = m["channel_indices"]
    balanced = c["out"].float()          # the recorded projection at strength 1: on the manifold up to fp32 rounding of the state
    mod = build(case, strength=strength)
    buf = {k: v.detach().cpu() for k, v in mod.named_buffers()}
    meta = dict(m, strength=strength)
    want = ref.projection_fwd(balanced, buf, meta)
    err32 = (ref.projection_fwd(balanced, buf, meta, dtype=torch.float32).double() - want).abs().max().item()
    y = mod(balanced.to(DEV)).cpu().double()
    gate = 2.0 * err32 + ulp32(want)
    assert (y - want).abs().max().item() <= gate
    # unchanged: the fp64 restatement itself moves the rounded state by no more than its rounding allows
    moved = (want - balanced.double()).abs().max().item()
    print(f"{case} strength {strength}: moved {(y - balanced.double()).abs().max().item():.3e} (fp64 {moved:.3e}, gate {gate:.3e})")
    assert (y - balanced.double()).abs().max().item() <= moved + gate
    assert torch.equal(y[:, [i for i in range(y.shape[1]) if i not in idx]], balanced.double()[:, [i for i in range(y.shape[1]) if i not in idx]])


# ---- reproducibility and graph capture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", LAYERS + ["wrapper_window_of_13", "nonneg_silu"])
def test_runs_are_bit_identical_and_replay_from_a_graph(case, dtype):
    c = CASES[case]
    mod = build(case)
    gen = torch.Generator().manual_seed(17)
    x = quantised((2, c["x"].shape[1], 6, 16), gen).to(dtype).to(DEV)
    g = quantised((2, c["g"].shape[1], 6, 16), gen).to(dtype).to(DEV)
    y0, g0 = run(mod, x, g)
    y1, g1 = run(mod, x, g)
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    xs = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up on the side stream, as capture asks for
        for _ in range(2):
            (w,) = torch.autograd.grad(mod(xs), xs, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yc = mod(xs)
        (gc,) = torch.autograd.grad(yc, xs, g)
    with torch.no_grad():
        xs.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    ye, ge = run(mod, x.flip(0), g)
    assert torch.equal(yc, ye) and torch.equal(gc, ge)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _wrapped_sfno():
    import json
    import makani_amd as ma
    c = CASES["wrapper_two_levels"]
    m = c["meta"]
    kwargs = json.loads(str(load_golden("sfno_posembed_direct_19x36.npz")["kwargs"]))          # the smallest network of the golden set
    params = dict(constraints=[{"type": "hydrostatic_balance", "options": m["kwargs"]}], channel_names=m["channel_names"],
                  N_out_channels=len(m["channel_names"]))
    kwargs.update(inp_chans=len(m["channel_names"]))
    handle, out_chans = ma.constrain_model_handle(params, lambda out_chans: ma.SphericalFourierNeuralOperatorNet(**dict(kwargs, out_chans=out_chans)),
                                                  c["bias"], c["scale"])
    assert out_chans == m["N_in_channels"]
    torch.manual_seed(12)
    model = handle().to(DEV)
    assert isinstance(model, ma.ConstraintsWrapper) and model.model.out_chans == out_chans
    return model, c


def _param_grads(model):
    return [p.grad.clone() for p in model.parameters() if p.grad is not None]


def test_constraints_wrapper_around_the_smallest_sfno():
    model, c = _wrapped_sfno()
    m = c["meta"]
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, len(m["channel_names"]), 19, 36, generator=gen).to(DEV)
    g = quantised((2, len(m["channel_names"]), 19, 36), gen).to(DEV)
    model.zero_grad(set_to_none=True)
    y = model(x)
    y.backward(g)
    got = _param_grads(model)
    assert len(got) > 0
    # the same network followed by the reference's formula in fp32 torch
    model.zero_grad(set_to_none=True)
    raw = model.model(x)
    buf = dict(model.constraint_list[0].named_buffers())
    want = ref.wrapper_fwd(raw, buf, m, dtype=torch.float32)
    want.backward(g)
    ref_grads = _param_grads(model)
    # the formula's own fp32 error on this very input, against its fp64 evaluation
    raw_c = raw.detach().cpu()
    buf_c = {k: v.cpu() for k, v in buf.items()}
    y64 = ref.wrapper_fwd(raw_c, buf_c, m)
    err32 = (want.detach().cpu().double() - y64).abs().max().item()
    gate = max(2.0 * err32 + ulp32(y64), 1e-5 * float(y64.abs().max()))
    e_out = (y.detach() - want.detach()).abs().max().item()
    print(f"end to end: out {e_out:.3e} (gate {gate:.3e})")
    assert e_out <= gate
    for a, b in zip(got, ref_grads):
        e, gate_p = (a - b).abs().max().item(), 1e-5 * float(b.abs().max()) + 2.0 ** -23 * float(b.abs().max())
        assert e <= gate_p, (e, gate_p, tuple(a.shape))


def test_wrapped_model_in_the_multistep_wrapper_with_and_without_checkpointing():
    import makani_amd as ma
    model, c = _wrapped_sfno()
    n = len(c["meta"]["channel_names"])
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(1, n, 19, 36, generator=gen).to(DEV)
    g = quantised((1, 2 * n, 19, 36), gen).to(DEV)

    def grads(checkpointed):
        model.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_(True)
        y = ma.MultiStepWrapper(model, n_future=1, multistep_checkpoint=checkpointed).train()(xs)
        assert y.shape == (1, 2 * n, 19, 36)
        y.backward(g)
        return y.detach(), xs.grad.clone(), _param_grads(model)

    plain, ckpt = grads(False), grads(True)
    assert torch.equal(plain[0], ckpt[0]) and torch.equal(plain[1], ckpt[1])
    assert len(plain[2]) == len(ckpt[2]) > 0 and all(torch.equal(a, b) for a, b in zip(plain[2], ckpt[2]))
