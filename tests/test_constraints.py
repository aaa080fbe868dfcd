"""The output constraints without a GPU: the fp64 restatement (tests/_constraints_ref.py) against tests/golden/constraints.npz,
recorded by tools/make_constraints_golden.py from the reference's own classes in double precision; what the constructors of
``makani_amd.constraints`` build; the reference's errors; ``state_dict`` compatibility; ``constrain_model_handle``; and the
argument validation of the C ABI.

Gates: the restatement reproduces the recorded output and gradient to 1e-12 relative to the largest recorded magnitude (both are
fp64 evaluations of the same formula on the same fp32 operators); constructed buffers equal the recorded ones to 1e-6 relative
(fp32 rounding of an fp64 construction)."""
import ctypes
import os
import sys
from functools import partial

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _constraints_ref as ref          # noqa: E402
from conftest import GOLDEN, load_golden          # noqa: E402

import makani_amd as ma          # noqa: E402
from makani_amd import constraints as mc          # noqa: E402

CASES = ref.load_cases(load_golden("constraints.npz"))
NAMES = sorted(CASES)


def build(case, **override):
    """the package's class for a fixture case, from the recorded names, kwargs and statistics"""
    c = CASES[case]
    m = c["meta"]
    kw = dict(m["kwargs"])
    bias, scale = c.get("bias"), c.get("scale")
    if m["kind"] == "projection":
        kw["climatology_offset"] = c["climatology_offset"] if kw["climatology_offset"] else None
    kw.update(override)
    cls = {"wrapper": mc._HydrostaticBalanceWrapper, "projection": mc.HydrostaticBalanceProjection, "nonneg": mc.NonNegativeConstraint}[m["kind"]]
    return cls(channel_names=m["channel_names"], bias=bias, scale=scale, **kw).train(m["training"])


def test_the_fixture_holds_the_cases_the_layers_need():
    kinds = {n: CASES[n]["meta"] for n in NAMES}
    assert {(m["moist"]) for m in kinds.values() if m["kind"] == "wrapper"} == {False, True}
    proj = {(m["moist"], m["strength"], m["kwargs"]["climatology_offset"]) for n, m in kinds.items() if n.startswith("projection_") and
            m["channel_names"] == kinds["projection_dry_s10"]["channel_names"]}
    assert proj == {(a, s, c) for a in (False, True) for s in (1.0, 0.7) for c in (False, True)}
    assert {(m["mode"], m["training"], m["with_stats"]) for m in kinds.values() if m["kind"] == "nonneg"} == \
        {(md, tr, st) for (md, tr) in (("silu", True), ("softplus", True), ("silu", False)) for st in (False, True)}
    assert len(kinds["wrapper_two_levels"]["pressures"]) == 2 and kinds["projection_two_levels"]["num_levels"] == 2
    wide = kinds["wrapper_window_of_13"]
    assert sum(n.startswith("z") for n in wide["channel_names"]) == 13 and 2 < len(wide["pressures"]) < 13
    assert wide["pressures"] == sorted(wide["pressures"], reverse=True) and wide["z_idx"] != sorted(wide["z_idx"])
    for n in NAMES:
        assert CASES[n]["x"].shape[0::2] == (2, 5) and CASES[n]["x"].shape[-1] == 7
        assert sum(v.numel() * v.element_size() for v in CASES[n].values() if isinstance(v, torch.Tensor)) < 100e3, n
    assert os.path.getsize(os.path.join(GOLDEN, "constraints.npz")) < 2 ** 20
    assert float(CASES["wrapper_dry"]["scale"].max()) > 2e3 and float(CASES["wrapper_dry"]["bias"].max()) > 3e4
    ev = CASES["nonneg_eval"]
    lo = -ev["buf"]["offset"].reshape(-1)
    assert (ev["x"][:, ev["meta"]["channel_indices"]] - lo.view(1, -1, 1, 1)).abs().min() >= 1e-3


@pytest.mark.parametrize("case", NAMES)
def test_restatement_reproduces_the_recorded_double_run(case):
    c = CASES[case]
    kind = c["meta"]["kind"]
    out = ref.FWD[kind](c["x"], c["buf"], c["meta"])
    grad = ref.BWD[kind](c["x"], c["g"], c["buf"], c["meta"])
    assert out.shape == c["out"].shape and grad.shape == c["grad"].shape
    assert (out - c["out"]).abs().max() <= 1e-12 * c["out"].abs().max()
    assert (grad - c["grad"]).abs().max() <= 1e-12 * c["grad"].abs().max()


@pytest.mark.parametrize("case", NAMES)
def test_constructors_build_the_recorded_buffers_and_indices(case):
    c = CASES[case]
    m = c["meta"]
    mod = build(case)
    bufs = dict(mod.named_buffers())
    assert sorted(bufs) == sorted(c["buf"])
    for name, want in c["buf"].items():
        got = bufs[name]
        assert got.dtype == want.dtype and got.shape == want.shape, name
        if want.dtype == torch.long:
            assert torch.equal(got, want), name
        else:
            assert (got.double() - want.double()).abs().max() <= 1e-6 * want.double().abs().max(), name
    assert sorted(mod.state_dict().keys()) == m["persistent"]
    if m["kind"] == "wrapper":
        assert (mod.z_idx, mod.t_idx, mod.aux_idx, mod.pressures) == (m["z_idx"], m["t_idx"], m["aux_idx"], m["pressures"])
        assert mod.mapping.shape[1] == m["N_in_channels"] and mod.use_moist_air_formula == m["moist"]
        if m["moist"]:
            assert mod.q_idx == m["q_idx"]
        cw = ma.ConstraintsWrapper([{"type": "hydrostatic_balance", "options": m["kwargs"]}], m["channel_names"], c.get("bias"), c.get("scale"))
        assert cw.N_in_channels == m["N_in_channels"] and cw.model is None and len(cw.constraint_list) == 1
    elif m["kind"] == "projection":
        assert mod.num_levels == m["num_levels"] and mod.strength == m["strength"]
    else:
        assert (mod.eps, mod.leak, mod.mode) == (m["eps"], m["leak"], m["mode"])


def test_channel_matching():
    names = CASES["wrapper_window_of_13"]["meta"]["channel_names"]
    z, t, p = mc.get_matching_channels_pl(names, "z", "t", 100, 900)
    assert p == [850, 700, 600, 500, 400, 300, 250, 200, 150, 100]
    assert [names[i] for i in z] == [f"z{q}" for q in p] and [names[i] for i in t] == [f"t{q}" for q in p]
    assert mc.get_matching_channels_pl(names, "z", "t", 100, 900, revert=False)[2] == p[::-1]
    assert mc.get_matching_channels_pl(["t2m", "tcwv", "z500", "t500"], "z", "t", 0, 1000) == ([2], [3], [500])


def test_the_errors_of_the_reference():
    names = CASES["wrapper_moist"]["meta"]["channel_names"]
    with pytest.raises(ValueError, match="need at least two overlapping z/t pressure levels"):
        mc.HydrostaticBalanceProjection(["z500", "t500", "t850"])
    with pytest.raises(ValueError, match="overlapping pressure levels for geopotential and temperature"):
        mc._HydrostaticBalanceWrapper(["z500", "t850"], None, None)
    with pytest.raises(ValueError, match="same pressure levels for t, z and q channels"):
        mc.HydrostaticBalanceProjection(["z500", "t500", "z850", "t850", "t250", "q250", "q500"], use_moist_air_formula=True)
    with pytest.raises(ValueError, match="same pressure levels for t,z and q channels"):
        mc._HydrostaticBalanceWrapper(["z500", "t500", "z850", "t850", "t250", "q250", "q500"], None, None, use_moist_air_formula=True)
    with pytest.raises(ValueError, match=r"climatology_offset must have length 2 \(one per interior level over all 3 matching"):
        mc.HydrostaticBalanceProjection(names, climatology_offset=torch.zeros(3))
    with pytest.raises(ValueError, match="mode must be 'silu' or 'softplus', got 'relu'"):
        mc.NonNegativeConstraint(names, ["q500"], mode="relu")
    with pytest.raises(ValueError, match="None of the requested channel names"):
        mc.NonNegativeConstraint(names, ["q123"])
    with pytest.raises(NotImplementedError, match="different from hydrostatic balance"):
        ma.ConstraintsWrapper([{"type": "mass_conservation", "options": {}}], names, None, None)


def test_more_than_sixteen_levels_raise_on_the_host():
    levels = [50 * i for i in range(1, 18)]
    names = [f"{v}{p}" for p in levels for v in ("z", "t")]
    with pytest.raises(ValueError, match="at most 16 levels"):
        mc._HydrostaticBalanceWrapper(names, None, None, p_min=0, p_max=2000)
    with pytest.raises(ValueError, match="at most 16 levels"):
        mc.HydrostaticBalanceProjection(names, p_min=0, p_max=2000)
    assert mc._HydrostaticBalanceWrapper(names, None, None, p_min=100, p_max=2000).num_levels == 16


@pytest.mark.parametrize("case", ["wrapper_dry", "wrapper_moist", "projection_moist_s07_clim", "nonneg_softplus"])
def test_strict_load_of_the_recorded_state_dict(case):
    c = CASES[case]
    state = {k: c["buf"][k].clone() for k in c["meta"]["persistent"]}
    other = build(case) if c["meta"]["kind"] != "wrapper" else mc._HydrostaticBalanceWrapper(c["meta"]["channel_names"], None, None,
                                                                                              **c["meta"]["kwargs"])
    res = other.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in state.items():
        assert torch.equal(dict(other.named_buffers())[k], v)
    if c["meta"]["kind"] == "wrapper":          # the constraint list of the wrapper carries the same keys one level down
        cw = ma.ConstraintsWrapper([{"type": "hydrostatic_balance", "options": c["meta"]["kwargs"]}], c["meta"]["channel_names"], None, None)
        cw.load_state_dict({f"constraint_list.0.{k}": v for k, v in state.items()}, strict=True)


def test_a_cpu_tensor_raises():
    for case in ("wrapper_dry", "projection_dry_s10", "nonneg_silu"):
        with pytest.raises(RuntimeError, match="GPU"):
            build(case)(CASES[case]["x"])


class _Params(dict):
    __getattr__ = dict.__getitem__


def test_constrain_model_handle_binds_a_recipe():
    c = CASES["wrapper_moist"]
    m = c["meta"]
    seen = {}

    class Net(torch.nn.Module):
        def __init__(self, inp_chans, out_chans):
            super().__init__()
            seen.update(inp_chans=inp_chans, out_chans=out_chans)

    params = _Params(constraints=[{"type": "hydrostatic_balance", "options": m["kwargs"]}], channel_names=m["channel_names"],
                     N_out_channels=len(m["channel_names"]))
    handle, out_chans = mc.constrain_model_handle(params, partial(Net, inp_chans=7, out_chans=len(m["channel_names"])), c["bias"], c["scale"])
    assert out_chans == m["N_in_channels"] < len(m["channel_names"])
    model = handle()
    assert isinstance(model, ma.ConstraintsWrapper) and isinstance(model.model, Net) and seen == dict(inp_chans=7, out_chans=out_chans)
    assert model.N_in_channels == out_chans
    assert torch.equal(model.constraint_list[0].out_bias, c["buf"]["out_bias"])
    same, n = mc.constrain_model_handle(_Params(N_out_channels=5), Net, None, None)
    assert same is Net and n == 5
    import makani_plugin
    assert makani_plugin.ConstraintsWrapper is ma.ConstraintsWrapper


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    from makani_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    f32 = _lib.MK_F32

    def fwd(x=p, y=p, it=p, ft=p, dt=f32, B=2, Cin=6, Cout=7, K_in=3, K_out=4, NQ=0, n_mi=0, n_mo=0, NC=3, flags=0, hw=4):
        return L.mk_cmix_fwd(x, y, dt, it, ft, B, Cin, Cout, K_in, K_out, NQ, n_mi, n_mo, NC, flags, 1.0, 0.6, hw, null)

    def bwd(g=p, x=null, gx=p, NQ=0, n_mo=0, Cin=6, Cout=7):
        return L.mk_cmix_bwd(g, x, gx, f32, p, p, 2, Cin, Cout, 3, 4, NQ, 0, n_mo, 3, 0, 1.0, 0.6, 4, null)

    for kwargs, what in ((dict(x=null), "null pointer"), (dict(y=null), "null pointer"), (dict(it=null), "null pointer"),
                         (dict(ft=null), "null pointer"), (dict(dt=5), "f32 or bf16"), (dict(B=0), "B = 0"), (dict(hw=0), "HW = 0"),
                         (dict(K_out=33, Cout=36), "at most 16 levels"), (dict(K_in=0, Cin=3), "K_in = 0"),
                         (dict(NQ=17, Cin=23, Cout=24), "NQ = 17"), (dict(n_mo=1), "n_mo = 1 moist rows next to NQ = 0"),
                         (dict(NC=2), "every channel is written once"), (dict(Cin=0), "must be positive"), (dict(flags=4), "flags = 4")):
        rc = fwd(**kwargs)
        assert rc < 0 and what in L.mk_last_error().decode(), (rc, what, L.mk_last_error().decode())
    assert bwd(g=null) < 0 and bwd(gx=null) < 0
    assert bwd(NQ=2, n_mo=2, Cin=8, Cout=9) < 0 and "null pointer" in L.mk_last_error().decode()          # the moist forms read x

    def nn(x=p, y=p, slot=p, dt=f32, mode=0, eps=0.1, B=2, C_=3, hw=4):
        return L.mk_nonneg_fwd(x, y, dt, slot, null, mode, eps, 0.02, B, C_, hw, null)

    for kwargs, what in ((dict(x=null), "null pointer"), (dict(y=null), "null pointer"), (dict(slot=null), "null pointer"),
                         (dict(dt=2), "f32 or bf16"), (dict(mode=3), "mode = 3"), (dict(eps=0.0), "eps = 0"), (dict(B=0), "B = 0"),
                         (dict(C_=70000), "C = 70000"), (dict(hw=-1), "HW = -1")):
        rc = nn(**kwargs)
        assert rc < 0 and what in L.mk_last_error().decode(), (rc, what, L.mk_last_error().decode())
    assert L.mk_nonneg_bwd(null, p, p, f32, p, null, 0, 0.1, 0.02, 2, 3, 4, null) < 0
    assert L.mk_nonneg_bwd(p, null, p, f32, p, null, 0, 0.1, 0.02, 2, 3, 4, null) < 0


def test_descriptor_rejects_channel_lists_that_do_not_partition():
    from makani_amd import ops
    one = torch.ones(2)
    with pytest.raises(ValueError, match="partition"):
        ops.column_mix([0, 1], [0, 1], [], [], [2], [3], one, one, one, one, None, None, None, torch.eye(2), 3, 3, 0, 0, True, False, -1.0,
                       0.0, "cpu")
    d = ops.column_mix([0, 1], [2, 0], [], [], [2], [1], one, one, one, one, None, None, None, torch.eye(2), 3, 3, 0, 0, True, False, -1.0,
                       0.0, "cpu")
    assert d.itab.numel() == 96 + 2 and d.ftab.numel() == 7 * 32 + 2 * 16 + 4 * 32 * 32 and d.itab[2:32].tolist() == [1] * 30 and d.NC == 1
