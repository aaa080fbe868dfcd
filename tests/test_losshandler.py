"""CPU tests of ``LossHandler``, ``HydrostaticBalanceLoss`` and ``DriftRegularization``: the fp64 restatement of
tests/_losshandler_ref.py against the values recorded from the reference (tests/golden/losshandler.npz, written by
tools/make_losshandler_golden.py), and what of the three classes does not need a GPU: registry, buffers, weights, errors.

The recorded values are the reference's fp32 CPU results on 9 x 16 planes: sums of 144 terms, each term a handful of fp32
operations, so 1e-5 relative (144 x 2^-24 = 8.6e-6, the worst case of recursive summation) bounds their distance from fp64."""
import json

import pytest
import torch

from _ranks import launch, ranks
from conftest import load_golden, rel_l2

import _losshandler_ref as ref
import makani_amd as ma
from makani_amd import losses as ml

G = load_golden("losshandler.npz")
CASES = ("l2_eval", "multistep", "mixed_dry", "mixed_moist", "balanced", "running_stats")
NAMES = "u10m t2m z500 z850 z1000 t500 t850 t1000 q500 q850 q1000".split()
KW = dict(img_shape=(9, 16), crop_shape=(9, 16), crop_offset=(0, 0), channel_names=NAMES, grid_type="equiangular")
TOL = 1e-5


def _meta(name):
    return json.loads(str(G[f"{name}/meta"]))


def _t(key):
    return torch.from_numpy(G[key])


def _ref_handler(name):
    meta = _meta(name)
    cmat = next((_t(k) for k in G.files if k.startswith(f"{name}/buf/") and k.endswith(".cmat")), None)
    h = ref.Handler(meta, _t("bias"), _t("scale"), _t("time_diff_stds"), cmat)
    if f"{name}/before/running_mean" in G.files:
        h.mean, h.m2 = _t(f"{name}/before/running_mean").double(), _t(f"{name}/before/running_var").double()
        h.count = int(G[f"{name}/before/num_batches_tracked"][0])
    return h


def _handler(name, **kw):
    meta = _meta(name)
    return ma.LossHandler(ref.params_of(meta), bias=_t("bias"), scale=_t("scale"), time_diff_stds=_t("time_diff_stds"),
                          **meta["handler_kwargs"], **kw).train(meta["training"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_recorded_reference(name):
    h = _ref_handler(name)
    if name == "running_stats":          # the first of its two updates
        h.mean, h.m2, h.count = torch.zeros_like(h.mean), torch.ones_like(h.m2), 0
        h(*ref.case_inputs(G, name, call=0))
    prd, tar, inp = ref.case_inputs(G, name)
    prd = prd.double().requires_grad_(True)
    loss, vec = h(prd, tar, inp)
    (grad,) = torch.autograd.grad(loss, prd)
    errs = {f"vec{i}": rel_l2(v, _t(f"{name}/vec{i}")) for i, v in enumerate(vec)}
    errs["loss"] = abs(loss.item() - float(G[f"{name}/loss"])) / abs(float(G[f"{name}/loss"]))
    errs["grad"] = rel_l2(grad, _t(f"{name}/grad"))
    assert rel_l2(h.chw, _t(f"{name}/buf/channel_weights")) <= 1e-7 and torch.equal(h.msw, _t(f"{name}/buf/multistep_weight"))
    if name in ("balanced", "running_stats"):
        errs["running_mean"] = rel_l2(h.mean, _t(f"{name}/buf/running_mean"))
        errs["running_var"] = rel_l2(h.m2, _t(f"{name}/buf/running_var"))
        assert h.count == int(G[f"{name}/buf/num_batches_tracked"][0])
    print(name, " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("moist", [False, True])
def test_written_out_hydrostatic_gradient_is_the_derivative_of_the_sums(moist):
    gen = torch.Generator().manual_seed(5)
    m = ma.HydrostaticBalanceLoss(bias=_t("bias"), scale=_t("scale"), p_min=400, use_moist_air_formula=moist, **KW)
    x = torch.randn(2, 11, 9, 16, generator=gen, dtype=torch.float64).requires_grad_(True)
    g, w = torch.randn(2, 2, generator=gen, dtype=torch.float64), torch.rand(2, 1, 9, 16, generator=gen, dtype=torch.float64)
    args = (_t("bias"), _t("scale"), m.cmat, m.z_idx, m.t_idx, m.q_idx if moist else None, ref.quad_weights(9, 16))
    (auto,) = torch.autograd.grad((ref.hydro_sums(x, *args, wgt=w) * g).sum(), x)
    assert rel_l2(ref.hydro_grad(x.detach(), *args, g, wgt=w), auto) <= 1e-13


def test_registry_names_and_types():
    assert sorted(ml._LOSS_REGISTRY) == sorted([
        "l1", "l2", "spectral l1", "spectral l2", "h1", "amse", "hydrostatic", "ensemble_crps", "ensemble_spectral_crps",
        "ensemble_vort_div_crps", "ensemble_gradient_crps", "ensemble_nll", "gaussian_mmd", "lp_energy_score", "l2_energy_score",
        "sobolev_energy_score", "spectral_l2_energy_score", "drift_regularization", "spectral_regularization"])
    assert ma.LossHandler is ml.LossHandler
    h = _handler("mixed_moist")
    assert h.loss_types == ["deterministic", "probabilistic", "probabilistic", "deterministic"]
    assert [{"deterministic": 1, "probabilistic": 2}[t] for t in h.loss_types] == _meta("mixed_moist")["loss_types"]
    assert h.loss_requires_input == [False, True, False, False] and not h.is_distributed()
    assert isinstance(h.loss_fn[3], ma.HydrostaticBalanceLoss) and isinstance(h.loss_fn[2], ma.DriftRegularization)
    for cls, kw in ((ma.GeometricLpLoss, {}), (ma.SpectralLpLoss, {}), (ma.SpectralH1Loss, {})):
        m = cls(**KW, **kw)
        assert m.type == "deterministic" and m.compute_channel_weighting("constant", time_diff_scale=None).tolist() == [1.0] * 11
    assert ma.SpectralCRPSLoss(**KW).type == "probabilistic" and ma.DriftRegularization(**KW).type == "probabilistic"


@pytest.mark.parametrize("name", CASES)
def test_buffers_and_state_dict_are_the_references(name):
    h = _handler(name)
    meta = _meta(name)
    assert sorted(h.state_dict()) == meta["persistent"] == ["num_batches_tracked", "running_mean", "running_var"]
    assert torch.equal(h.channel_weights, _t(f"{name}/buf/channel_weights"))
    assert torch.equal(h.multistep_weight, _t(f"{name}/buf/multistep_weight"))
    state = {k: _t(f"{name}/before/{k}") for k in meta["persistent"]}
    h.load_state_dict(state, strict=True)
    assert h.num_batches_tracked.dtype == torch.long and torch.equal(h.running_var, state["running_var"])
    h.reset_running_stats()
    assert int(h.num_batches_tracked) == 0 and bool((h.running_var == 1).all()) and bool((h.running_mean == 0).all())


def test_hydrostatic_buffers_are_bit_equal_to_the_recorded_ones():
    for name, moist in (("mixed_dry", False), ("mixed_moist", True)):
        m = ma.HydrostaticBalanceLoss(bias=_t("bias"), scale=_t("scale"), p_min=400, use_moist_air_formula=moist, **KW)
        assert torch.equal(m.cmat, _t(f"{name}/buf/loss_fn.3.cmat")) and torch.equal(m.p, _t(f"{name}/buf/loss_fn.3.p"))
        assert m.n_channels == 2 and m.type == "deterministic" and list(m.state_dict()) == []
        assert sorted(n for n, _ in m.named_buffers() if "." not in n) == ["bias", "cmat", "p", "scale"]
        assert m.compute_channel_weighting("constant", time_diff_scale=None).tolist() == [0.5, 0.5]
        with pytest.raises(NotImplementedError):
            m.compute_channel_weighting("auto")
        with pytest.raises(NotImplementedError):
            m.compute_channel_weighting("constant", time_diff_scale=torch.ones(2))


def test_hydrostatic_errors():
    b, s = torch.zeros(1, 3, 1, 1), torch.ones(1, 3, 1, 1)
    with pytest.raises(ValueError, match="at least two pressure levels"):
        ma.HydrostaticBalanceLoss((9, 16), (9, 16), (0, 0), ["z500", "t500", "u10m"], "equiangular", b, s)
    with pytest.raises(ValueError, match="same pressure levels for t,z and q"):
        ma.HydrostaticBalanceLoss((9, 16), (9, 16), (0, 0), [f"{v}{p}" for v in "zt" for p in (500, 850)] + ["q500", "q700"], "equiangular",
                                  torch.zeros(1, 6, 1, 1), torch.ones(1, 6, 1, 1), use_moist_air_formula=True)
    names = [f"{v}{p}" for v in "zt" for p in range(100, 1000, 50)][:36]
    lv = sorted({int(n[1:]) for n in names})
    names17 = [f"{v}{p}" for v in "zt" for p in lv[:17]]
    with pytest.raises(ValueError, match="at most 16 levels"):
        ma.HydrostaticBalanceLoss((9, 16), (9, 16), (0, 0), names17, "equiangular", torch.zeros(1, 34, 1, 1), torch.ones(1, 34, 1, 1))
    m = ma.HydrostaticBalanceLoss(bias=_t("bias"), scale=_t("scale"), **KW)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(2, 11, 9, 16), None)


def test_multistep_weights_and_their_errors():
    meta = dict(_meta("l2_eval"), n_future=3)
    want = {"constant": [0.25] * 4, "balanced": [0.1, 0.2, 0.3, 0.4], "linear": [0.25, 0.5, 0.75, 1.0], "last-n-1": [0.0, 1 / 3, 1 / 3, 1 / 3],
            "last": [0.0, 0.0, 0.0, 1.0], "custom": [0.5, 0.25, 0.125, 0.125]}
    for kind, w in want.items():
        ms = dict(weight_type=kind, **({"weights": w} if kind == "custom" else {}))
        h = ma.LossHandler(ref.params_of(dict(meta, multistep=ms)))
        assert h.multistep_weight.shape == (1, 44)
        assert torch.allclose(h.multistep_weight.reshape(4, 11), torch.tensor(w).reshape(4, 1).expand(4, 11), rtol=1e-7, atol=0)
        assert h.running_mean.shape == (44,)
    with pytest.raises(ValueError, match=r"Number of multistep weights \(2\) must match n_future\+1 \(4\)"):
        ma.LossHandler(ref.params_of(dict(meta, multistep=dict(weight_type="custom", weights=[0.5, 0.5]))))
    with pytest.raises(ValueError, match="Unknown multistep loss weight type: cubic"):
        ma.LossHandler(ref.params_of(dict(meta, multistep=dict(weight_type="cubic"))))


def test_handler_errors():
    meta = _meta("l2_eval")
    p = ref.params_of(meta)
    del p.losses
    with pytest.raises(ValueError, match="No loss function specified."):
        ma.LossHandler(p)
    p.loss = "l2"
    assert isinstance(ma.LossHandler(p, compile=True).loss_fn[0], ma.GeometricLpLoss)
    with pytest.raises(NotImplementedError, match="Unknown loss function: l3"):
        ma.LossHandler(ref.params_of(dict(meta, losses=[{"type": "l3"}])))
    with pytest.raises(ValueError, match="expected channel weights to have 11 channels, but got 3"):
        ma.LossHandler(ref.params_of(dict(meta, losses=[{"type": "l2", "channel_weights": [[1.0, 2.0, 3.0]]}])))
    h = ma.LossHandler(ref.params_of(dict(meta, losses=[{"type": "l2", "channel_weights": [[float(i) for i in range(11)]], "relative_weight": 2.0}])))
    assert h.channel_weights.tolist() == [[2.0 * i for i in range(11)]]
    p = ref.params_of(meta)
    p.random_slice_loss = True
    with pytest.raises(NotImplementedError, match="random_slice_loss"):
        ma.LossHandler(p)
    with pytest.raises(ValueError, match="time_diff_std_path not defined."):
        ma.LossHandler(ref.params_of(dict(meta, losses=[{"type": "l2", "temp_diff_normalization": True}])))
    h = _handler("l2_eval")
    with pytest.raises(ValueError, match="Module does not track running stats"):
        h.get_running_stats()
    with pytest.raises(RuntimeError, match="GPU"):
        h(torch.zeros(2, 3, 11, 9, 16), torch.zeros(2, 11, 9, 16))


def test_a_loss_asked_directly_answers_as_before():
    """the handler's normalised weights do not leak: outside it a loss returns the project's plain weights, and a
    time-difference scale stays an error"""
    _handler("mixed_dry")
    m = ma.GeometricLpLoss(**KW)
    assert m.compute_channel_weighting("auto").tolist() == pytest.approx([0.1, 1.0, 0.5, 0.85, 1.0, 0.5, 0.85, 1.0, 0.5, 0.85, 1.0])
    with pytest.raises(NotImplementedError):
        ma.CRPSLoss(**KW).compute_channel_weighting("auto", time_diff_scale=torch.ones(11))


# ---- the running statistics over the "batch" group: two CPU ranks over gloo (the update is plain torch) ------------------------
def _batch_worker(rank, world, rendezvous):
    with ranks(rank, world, rendezvous):
        import makani_amd.comm as mcomm
        mcomm.init(1, 1)
        assert mcomm.get_size("batch") == world and mcomm.get_rank("batch") == rank
        h = _handler("running_stats")
        x = torch.randn(2, 3, 22, generator=torch.Generator().manual_seed(8)).double().float()          # (update, rank * 2 rows, n)
        whole = ref.Handler(_meta("running_stats"), _t("bias"), _t("scale"), _t("time_diff_stds"))
        for u in range(2):
            rows = torch.stack([x[u, 0] * (r + 1) + x[u, 1] for r in range(2 * world)])          # the 4 rows of the global batch
            h._update_running_stats(rows[2 * rank:2 * rank + 2].clone())
            whole.update(rows)
        assert int(h.num_batches_tracked) == 4 * 2 == whole.count
        assert rel_l2(h.running_mean, whole.mean) <= 1e-6 and rel_l2(h.running_var, whole.m2) <= 1e-6
        mcomm.reset()


def test_running_statistics_are_gathered_over_the_batch_group():
    launch(_batch_worker, 2, limit=240)
