"""The geometric validation metrics (makani_amd/metrics.py, csrc/metrics.hip) without a GPU: the fp64 restatement of
tests/_metrics_ref.py against fixtures recorded in double precision from the reference's own classes
(tools/make_metrics_golden.py), the ``compute_counts`` / ``combine`` / ``finalize`` of the package's classes against the
recorded reference values, the constructor and error contract, and the host-side validation of the two entry points."""
import ctypes
import inspect
import os

import pytest
import torch

import _metrics_ref as ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["l1", "l1_weights_normalize", "rmse", "rmse_weights", "rmse_crop_normalize", "acc_macro", "acc_micro", "acc_macro_bias_weights",
         "acc_micro_bias", "acc_crop_bias", "spread_e3", "spread_e2_weights", "spread_e1", "ssr_e3", "ssr_e2_weights_crop", "ssr_e1",
         "crps_e3", "crps_e2_weights", "crps_e1", "rankhist_e3", "rankhist_e2_weights_normalize", "rankhist_e1", "rankhist_e3_crop"]
CLASSES = ["GeometricL1", "GeometricRMSE", "GeometricACC", "GeometricSpread", "GeometricSSR", "GeometricCRPS", "GeometricRankHistogram"]
KW = dict(grid_type="equiangular", img_shape=(17, 32), crop_shape=(17, 32), crop_offset=(0, 0))
TOL = 1e-12
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(ref.load_cases(load_golden("metrics.npz")))
    return _CASES


def build(c, cr, br):
    import makani_amd as ma
    kw = dict(c["kwargs"], channel_reduction=cr, batch_reduction=br)
    if c["bias"] is not None:
        kw["bias"] = c["bias"]
    return getattr(ma, c["cls"])(**kw)


@pytest.mark.parametrize("name", NAMES)
def test_fp64_restatement_matches_the_reference_fixtures(name):
    c = cases()[name]
    q = c["quad_weight"].double()
    for (cr, br), rec in c["variants"].items():
        kw = dict(c["kwargs"], channel_reduction=cr, batch_reduction=br)
        for a, want in ((c["a"], rec["out"]), (c["a"] + c["scale"], rec["out2"])):
            out = ref.metric(c["cls"], kw, a, c["b"], q, c["weights"], c["bias"])
            err = ref.mismatch(out, want)
            print(f"{name} {cr}-{br}: {err:.2e}")
            assert want.dtype == torch.float64 and out.shape == want.shape and err <= TOL, (name, cr, br, err)


def test_the_fixture_covers_what_it_should():
    import makani_amd as ma
    cs = cases()
    assert sorted(cs) == sorted(NAMES) and sorted({c["cls"] for c in cs.values()}) == sorted(CLASSES)
    all9 = {(cr, br) for cr in ("none", "mean", "sum") for br in ("none", "mean", "sum")}
    for cls in CLASSES:          # every class: all nine reductions, weights, and (ensemble classes) E = 1, 2, 3
        mine = [c for c in cs.values() if c["cls"] == cls]
        assert any(set(c["variants"]) == all9 for c in mine), cls
        assert any(c["weights"] is not None for c in mine), cls
        if mine[0]["E"]:
            assert {c["E"] for c in mine} == {1, 2, 3}, cls
    assert {c["kwargs"].get("method", "macro") for c in cs.values() if c["cls"] == "GeometricACC"} == {"macro", "micro"}
    assert any(c["bias"] is not None and c["kwargs"].get("method") == "micro" for c in cs.values())
    assert {bool(c["kwargs"].get("normalize", False)) for c in cs.values()} == {False, True}
    assert sum(tuple(c["kwargs"].get("crop_shape", (17, 32))) == (9, 20) for c in cs.values()) >= 3
    # one member: spread and SSR are 0 / 0
    assert bool(torch.isnan(cs["spread_e1"]["variants"][("none", "none")]["out"]).all())
    assert bool(torch.isnan(cs["ssr_e1"]["variants"][("none", "none")]["out"]).all())
    # ties: the observation equals one member, equals several members, lies below all and above all of them
    f, o = cs["rankhist_e3"]["a"], cs["rankhist_e3"]["b"]
    eq = (f == o.unsqueeze(1)).sum(dim=1)
    assert int((eq == 1).sum()) > 50 and int((eq >= 2).sum()) > 10
    assert int((f > o.unsqueeze(1)).all(dim=1).sum()) > 50 and int((f < o.unsqueeze(1)).all(dim=1).sum()) > 50
    # every bin of every histogram is occupied, so a rank off by one (side="left") cannot hide in an empty bin
    assert float(cs["rankhist_e3"]["variants"][("none", "none")]["out"].min()) > 0
    # the package's quadrature weights are the reference's, bit for bit (normalize, crop)
    for name in ("rmse", "rmse_crop_normalize", "rankhist_e3_crop", "l1_weights_normalize"):
        m = build(cs[name], "mean", "mean")
        assert torch.equal(m.quadrature.quad_weight[0, 0], cs[name]["quad_weight"]), name
    assert isinstance(build(cs["crps_e3"], "mean", "mean").metric_func, ma.CRPSLoss)


def test_a_rank_on_the_other_side_of_a_tie_misses_the_fixture():
    """the record distinguishes #{f <= o} (searchsorted side="right") from #{f < o}"""
    c = cases()["rankhist_e3"]
    f, o, q = c["a"].double(), c["b"].double(), c["quad_weight"].double()
    r = (f < o.unsqueeze(1)).sum(dim=1)
    left = torch.stack([(q * (r == k)).sum(dim=(-2, -1)) for k in range(4)], dim=-1)
    assert ref.mismatch(left, c["variants"][("none", "none")]["out"]) > 1e-2


@pytest.mark.parametrize("name", NAMES)
def test_counts_combine_and_finalize_match_the_reference(name):
    c = cases()[name]
    checked = 0
    for (cr, br), rec in c["variants"].items():
        if rec["counts"] is None:
            continue
        m = build(c, cr, br)
        if c["weights"] is None:          # (with weights the counts are a quadrature: tests/test_gpu_metrics.py)
            counts = m.compute_counts(c["a"].double(), None)
            assert counts.shape == rec["counts"].shape and torch.equal(counts, rec["counts"]), (name, cr, br)
        vals = torch.stack([rec["out"], rec["out2"]], dim=0)
        cnts = torch.stack([rec["counts"], 2.0 * rec["counts"]], dim=0)
        cv, cc = m.combine(vals, cnts, dim=0)
        assert cv.shape == rec["comb_vals"].shape and cc.shape == rec["comb_counts"].shape
        assert ref.mismatch(cv, rec["comb_vals"]) <= TOL and ref.mismatch(cc, rec["comb_counts"]) <= TOL, (name, cr, br)
        fin = m.finalize(rec["comb_vals"], rec["comb_counts"])
        assert fin.shape == rec["final"].shape and ref.mismatch(fin, rec["final"]) <= TOL, (name, cr, br)
        checked += 1
    assert checked or all(br == "none" for _, br in c["variants"]) or c["weights"] is not None


def test_constructor_contract():
    import makani_amd as ma
    from makani_amd import metrics as mm
    assert (mm.LossType.Deterministic, mm.LossType.Probabilistic) == (1, 2)          # base_loss.py:244-246
    types = dict(GeometricL1=1, GeometricRMSE=1, GeometricACC=1, GeometricSpread=2, GeometricSSR=2, GeometricCRPS=2, GeometricRankHistogram=2)
    for cls in CLASSES:
        m = getattr(ma, cls)(**KW)
        sig = inspect.signature(getattr(ma, cls).__init__).parameters
        assert m.type == types[cls], cls
        assert (m.channel_reduction, m.batch_reduction) == ("mean", "mean") and len(m.state_dict()) == 0, cls
        assert sig["channel_reduction"].default == "mean" and sig["batch_reduction"].default == "mean" and "kwargs" in sig
        assert sig["spatial_distributed"].default is False
        total = float(m.quadrature.quad_weight.sum())
        if cls == "GeometricCRPS":          # functions.py:466-474: always normalised; crop arguments without defaults
            assert abs(total - 1.0) < 1e-6 and "normalize" not in sig and sig["crps_type"].default == "skillspread"
        else:
            assert sig["normalize"].default is False and abs(total - 4 * torch.pi) < 1e-4, cls
            assert not m.spatial_distributed
        if cls in ("GeometricCRPS", "GeometricRankHistogram"):
            assert sig["crop_shape"].default is inspect.Parameter.empty and sig["crop_offset"].default is inspect.Parameter.empty
        else:
            assert sig["crop_shape"].default is None and sig["crop_offset"].default == (0, 0)
        if cls in ("GeometricSSR", "GeometricCRPS", "GeometricRankHistogram"):
            assert sig["ensemble_distributed"].default is False
    assert inspect.signature(mm.GeometricBaseMetric.__init__).parameters["normalize"].default is True          # base_metric.py:79
    acc = ma.GeometricACC(**KW)
    assert (acc.method, acc.eps) == ("macro", 1e-8) and not hasattr(acc, "bias")
    assert ma.GeometricACC(bias=torch.ones(3, 17, 32), **KW).bias.shape == (3, 17, 32)
    assert ma.GeometricSSR(**KW).eps == 1e-6 and not ma.GeometricSSR(ensemble_distributed=True, **KW).ensemble_distributed
    rh = ma.GeometricRankHistogram(**KW)
    assert rh.quad_weight_split.shape == (1, 1, 544, 1) and not rh.ensemble_distributed
    # counts: (C,) or a scalar, a trailing axis for the micro ACC and the histogram; ensemble classes count dim 2
    x, f = torch.zeros(4, 3, 17, 32), torch.zeros(4, 2, 5, 17, 32)
    assert ma.GeometricL1(**dict(KW, channel_reduction="none", batch_reduction="sum")).compute_counts(x).tolist() == [4.0] * 3
    assert ma.GeometricACC(method="micro", **KW).compute_counts(x).shape == (1,)
    assert ma.GeometricRankHistogram(**dict(KW, channel_reduction="none")).compute_counts(f).shape == (5, 1)
    assert ma.GeometricSpread(**dict(KW, channel_reduction="sum", batch_reduction="sum")).compute_counts(f).item() == 20.0
    assert ma.GeometricCRPS(**dict(KW, channel_reduction="none")).compute_counts(f).tolist() == [1.0] * 5


def test_errors_on_cpu_tensors():
    import makani_amd as ma
    from makani_amd import metrics as mm
    x, f4, f5 = torch.zeros(2, 3, 17, 32), torch.zeros(2, 3, 17, 32), torch.zeros(2, 2, 3, 17, 32)
    for cls in ("GeometricSpread", "GeometricSSR", "GeometricCRPS", "GeometricRankHistogram"):
        with pytest.raises(ValueError, match="Error, forecasts tensor expected to have 5 dimensions but found 4."):
            getattr(ma, cls)(**KW)(f4, x)
    for cls in ("GeometricCRPS", "GeometricRankHistogram"):
        with pytest.raises(ValueError, match=r"the weights have to have the same number of dimensions \(found 2\) as observations \(found 4\)."):
            getattr(ma, cls)(**KW)(f5, x, torch.ones(17, 32))
    for cls in CLASSES:
        inp = f5 if cls in CLASSES[3:] else x
        with pytest.raises(ValueError, match="Batch reduction mode 'mean' is not supported when weights are provided. Use 'sum' instead."):
            getattr(ma, cls)(**KW).compute_counts(inp, torch.ones_like(x))
        with pytest.raises(ValueError, match="Batch reduction mode 'none' is not supported"):
            getattr(ma, cls)(**dict(KW, batch_reduction="none")).compute_counts(inp, torch.ones_like(x))
        with pytest.raises(RuntimeError, match="GPU"):          # no CPU fallback
            getattr(ma, cls)(**KW)(inp, x)
    with pytest.raises(RuntimeError, match="GPU"):
        ma.deterministic_sums(x, x, ma.GeometricL1(**KW).quadrature)
    for cls in ("GeometricSpread", "GeometricSSR", "GeometricRankHistogram"):
        with pytest.raises(NotImplementedError, match="ensemble size 33"):
            getattr(ma, cls)(**KW)(torch.zeros(1, 33, 3, 17, 32), x[:1])
    with pytest.raises(ValueError, match="without a batch axis"):
        ma.GeometricACC(bias=torch.zeros(2, 3, 17, 32), **KW)(x, x)
    with pytest.raises(ValueError, match="holds 544 weights"):
        ma.deterministic_sums(x[..., :9, :], x[..., :9, :], ma.GeometricL1(**KW).quadrature)
    m = ma.GeometricL1(**KW)
    with pytest.raises(ValueError, match="The shape of vals and counts have to match or be one"):
        m.combine(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="The shape of counts has to be exactly 1"):
        m.combine(torch.zeros(2, 3, 4), torch.zeros(2, 3))
    v, cnt = mm._sanitize_shapes(torch.zeros(2, 3, 4), torch.ones(3), dim=1)
    assert cnt.shape == (1, 3, 1)


def test_entry_points_validate_their_arguments_on_the_host():
    from makani_amd._lib import lib
    L, p, null = lib(), ctypes.c_void_p(64), ctypes.c_void_p(0)

    def det(x=p, y=p, q=p, out=p, ws=p, xd=0, yd=0, B=1, C=1, n=4, which=31):
        return L.mk_metric_det_sums(x, xd, y, yd, null, null, q, out, ws, B, C, n, which, None)

    def ens(f=p, o=p, q=p, out=p, ws=p, fd=0, B=1, E=2, C=1, n=4, which=7):
        return L.mk_metric_ens_sums(f, fd, o, null, q, out, ws, B, E, C, n, which, None)

    for kw in (dict(x=null), dict(y=null), dict(q=null), dict(out=null), dict(ws=null)):
        assert det(**kw) < 0 and b"metric_det_sums: null pointer" in L.mk_last_error(), kw
    for kw in (dict(f=null), dict(o=null), dict(q=null), dict(out=null), dict(ws=null)):
        assert ens(**kw) < 0 and b"metric_ens_sums: null pointer" in L.mk_last_error(), kw
    for n in (0, -4):
        assert det(n=n) < 0 and b"points per plane must be positive" in L.mk_last_error()
        assert ens(n=n) < 0 and b"points per plane must be positive" in L.mk_last_error()
    for E in (0, -1, 33):
        assert ens(E=E) < 0 and f"ensemble size {E} outside 1 <= E <= 32".encode() in L.mk_last_error()
    assert det(B=0) < 0 and b"must be positive" in L.mk_last_error()
    assert ens(C=0) < 0 and b"must be positive" in L.mk_last_error()
    assert det(B=256, C=256) < 0 and b"plane limit of 65535" in L.mk_last_error()
    assert ens(B=256, C=256) < 0 and b"plane limit of 65535" in L.mk_last_error()
    assert det(xd=2) < 0 and b"f32 or bf16" in L.mk_last_error()
    assert det(yd=-1) < 0 and b"f32 or bf16" in L.mk_last_error()
    assert ens(fd=2) < 0 and b"f32 or bf16" in L.mk_last_error()
    for which in (0, 32):
        assert det(which=which) < 0 and b"selects no sum or an unknown one" in L.mk_last_error()
    for which in (0, 8):
        assert ens(which=which) < 0 and b"selects no sum or an unknown one" in L.mk_last_error()
    assert [L.mk_metric_chunks(n) for n in (1, 126, 1024, 1025, 16380, 721 * 1440)] == [1, 1, 1, 2, 16, 64]


def test_header_and_library_agree():
    """(entry points, parameter types and the MK_METRIC_* values: tests/test_abi.py)"""
    from makani_amd import metrics as mm
    assert mm.SUM_ALL == 31 and mm.SUM_ACC == 28
    src = open(os.path.join(ROOT, "makani_amd", "csrc", "metrics.hip")).read()
    assert src.startswith("// MK_HIPCC_FLAGS: -fno-slp-vectorize") and "atomic" not in src.replace("no atomics", "")
