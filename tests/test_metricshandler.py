"""``MetricsHandler`` without a GPU.

* The fp64 restatement of tests/_mhandler_ref.py reproduces what the reference's own, unmodified ``MetricsHandler`` recorded in
  tests/golden/metricshandler.npz (tools/make_metricshandler_golden.py): every handle's curve and counter after every update,
  the finalized curves, the ACC integral and the scalar log entries, to <= 1e-6 (relative L2 per recorded array, the project's
  measure ``_metrics_ref.mismatch``; relative error per scalar log entry); counts are exact where the reference's are integers.
* A handler built on ``device="cpu"`` has the reference's handle names, channel lists, buffer shapes, aliases, report keys and
  errors; a CPU ``update`` raises ``RuntimeError``.
* The inputs of tests/test_gpu_mrollout.py let the reference FORMULA in plain fp32 torch (mean over the members, differences,
  sort + searchsorted + one_hot, the sorted skill / spread form of the CRPS) meet the GPU gate of 1e-5 against the restatement,
  so that gate tests the kernels and not cancellation."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _crps_ref
import _metrics_ref as ref
import _mhandler_ref as mh
import _mrollout_cases as cases
from _losshandler_ref import Params
from conftest import load_golden

TOL_GOLDEN, TOL_GPU = 1e-6, 1e-5
ALIASES = {"RMSE": "rmse_curve", "ACC": "acc_curve", "CRPS": "crps_curve", "SSR": "ssr_curve", "Rank Histogram": "rh_curve"}


@pytest.fixture(scope="module")
def golden():
    return load_golden("metricshandler.npz")


def _names():
    return mh.case_names(np.load(__file__.rsplit("/", 1)[0] + "/golden/metricshandler.npz"))


def test_the_fixture_holds_the_seven_cases(golden):
    assert sorted(mh.case_names(golden)) == sorted(["full", "deterministic", "weights", "nan", "wb2", "noclim", "absent"])
    meta = {n: mh.case_meta(golden, n) for n in mh.case_names(golden)}
    assert meta["full"]["E"] == 3 and len(meta["full"]["handles"]) == 7 and meta["full"]["calls"] == 6
    assert meta["deterministic"]["E"] == 1 and [h["name"] for h in meta["deterministic"]["handles"]] == ["L1", "RMSE", "ACC"]
    assert meta["weights"]["weights"] and not meta["noclim"]["climatology"] and meta["wb2"]["handler_kwargs"]["wb2_compatible"]
    assert [k for k in golden.files if k.endswith("/nan")] == [f"nan/call{c}/nan" for c in (3, 4, 5)]
    assert "w300" in meta["absent"]["handler_kwargs"]["l1_var_names"] and "w300" not in meta["absent"]["channel_names"]


@pytest.mark.parametrize("name", _names())
def test_the_restatement_reproduces_the_recorded_reference(golden, name):
    meta, h = mh.case_meta(golden, name), mh.case_handler(golden, name)
    assert [(n, ch) for n, ch, _ in h.handles] == [(d["name"], d["channels"]) for d in meta["handles"]]
    worst = 0.0
    for call in range(meta["calls"]):
        prd, tar, loss, idt, wgt = mh.case_call(golden, name, call)
        h.update(prd, tar, loss, idt, wgt)
        for d in meta["handles"]:
            curve = torch.from_numpy(golden[f"{name}/call{call}/{d['name']}/curve"])
            counter = torch.from_numpy(golden[f"{name}/call{call}/{d['name']}/counter"])
            assert list(curve.shape) == d["curve"] == list(h.curve[d["name"]].shape)
            assert list(counter.shape) == d["counter"] == list(h.counter[d["name"]].shape)
            errs = ref.mismatch(curve, h.curve[d["name"]]), ref.mismatch(counter, h.counter[d["name"]])
            worst = max(worst, *errs)
            assert max(errs) <= TOL_GOLDEN, (name, call, d["name"], errs)
            if bool((counter == counter.round()).all()):          # the reference counted samples: exact
                assert torch.equal(counter.double(), h.counter[d["name"]]), (name, call, d["name"])
    final, integral, logs = h.finalize()
    for d in meta["handles"]:
        err = ref.mismatch(torch.from_numpy(golden[f"{name}/final/{d['name']}"]), final[d["name"]])
        worst = max(worst, err)
        assert err <= TOL_GOLDEN, (name, d["name"], err)
    err = ref.mismatch(torch.from_numpy(golden[f"{name}/integral/ACC"]), integral["ACC"])
    assert err <= TOL_GOLDEN, (name, "integral", err)
    keys, vals = meta["log_keys"], golden[f"{name}/logs"]
    assert list(logs["metrics"]) == keys
    mine = [logs["base"]["validation steps"], logs["base"]["validation loss"]] + [logs["metrics"][k] for k in keys]
    lerr = max(abs(a - b) / abs(b) for a, b in zip(mine, vals))
    print(f"{name}: curves / counters / finalized {worst:.2e}, integral {err:.2e}, log entries {lerr:.2e}")
    assert mine[0] == vals[0] and lerr <= TOL_GOLDEN, (name, lerr)


def _params(meta, **extra):
    keys = ("channel_names", "dt", "dhours", "split_data_channels", "img_shape_x_resampled", "img_shape_y_resampled",
            "img_crop_offset_x", "img_crop_offset_y", "model_grid_type", "ensemble_size", "log_to_screen", "log_to_wandb")
    return Params(**dict({k: meta[k] for k in keys}, **extra))


@pytest.mark.parametrize("name", _names())
def test_a_cpu_handler_has_the_references_handles_buffers_aliases_and_report_keys(golden, name):
    import makani_amd as ma
    meta = mh.case_meta(golden, name)
    clim = torch.zeros(1, len(meta["channel_names"]), 9, 16) if meta["climatology"] else None
    h = ma.MetricsHandler(_params(meta), clim, meta["steps"], "cpu", scale=torch.from_numpy(golden["scale"]), **meta["handler_kwargs"])
    assert (h.dtxdh, h.dd) == (meta["dtxdh"], meta["dd"])
    assert [m.metric_name for m in h.metric_handles] == [d["name"] for d in meta["handles"]]
    base = h.metric_handles[0].rollout_curve.untyped_storage().data_ptr()
    for m, d in zip(h.metric_handles, meta["handles"]):
        assert m.metric_channels == d["channels"] and m.channel_mask == [meta["channel_names"].index(c) for c in d["channels"]]
        assert list(m.rollout_curve.shape) == d["curve"] and list(m.rollout_counter.shape) == d["counter"]
        assert m.rollout_curve_cpu.shape == m.rollout_curve.shape and m.rollout_curve.dtype == torch.float32
        assert m.rollout_curve.untyped_storage().data_ptr() == base == m.rollout_counter.untyped_storage().data_ptr()      # one allocation
        assert m.type == (ma.metrics.LossType.Deterministic if d["name"] in ("L1", "RMSE", "ACC") else ma.metrics.LossType.Probabilistic)
        if d["name"] in ALIASES:
            assert getattr(h, ALIASES[d["name"]]) is m.rollout_curve
        assert hasattr(m, "scale") == (d["name"] in ("RMSE", "CRPS", "Spread"))
        if hasattr(m, "scale"):
            assert torch.equal(m.scale, torch.from_numpy(golden["scale"]).reshape(-1)[m.channel_mask])
    assert h._shared_quadrature
    h.initialize_buffers()
    h.zero_buffers()
    logs = h.finalize()
    assert [k for k in logs["metrics"] if k != "rollouts"] == meta["log_keys"] and list(logs["base"]) == ["validation steps", "validation loss"]
    table = logs["metrics"]["rollouts"]
    if isinstance(table, dict):
        assert table["columns"] == ["metric type", "variable name", "time [h]", "value"]
        assert len(table["data"]) == sum(meta["steps"] * len(d["channels"]) for d in meta["handles"] if d["name"] != "Rank Histogram")
    assert set(h.curves()) == {d["name"] for d in meta["handles"]}
    with pytest.raises(NotImplementedError):
        h.save("metrics.h5")


def test_errors(golden):
    import makani_amd as ma
    meta = mh.case_meta(golden, "full")
    with pytest.raises(NotImplementedError, match="split_data_channels"):
        ma.MetricsHandler(_params(meta, split_data_channels=True), None, 3, "cpu")
    with pytest.raises(ValueError, match="weatherbench2 compatibility only supported on equiangular grids"):
        ma.MetricsHandler(_params(meta, model_grid_type="legendre-gauss"), None, 3, "cpu", wb2_compatible=True)
    handle = partial(ma.GeometricL1, grid_type="equiangular", img_shape=(9, 16), channel_reduction="none", batch_reduction="none")
    with pytest.raises(ValueError, match="Batch reduction mode 'none' is not supported for rollout handlers"):
        ma.MetricRollout("L1", ["t2m"], handle, meta["channel_names"], 3, 6, "cpu")
    with pytest.raises(ValueError, match="scale holds"):
        ma.MetricsHandler(_params(meta), None, 3, "cpu", scale=torch.ones(3))
    h = ma.MetricsHandler(_params(meta), None, 3, "cpu", **meta["handler_kwargs"])
    h.initialize_buffers()
    C = len(meta["channel_names"])
    with pytest.raises(ValueError, match="at least two members"):          # a CRPS handle and a deterministic prediction
        h.update(torch.zeros(2, C, 9, 16), torch.zeros(2, C, 9, 16), torch.zeros(()), 0)
    with pytest.raises(ValueError, match="at least two members"):
        h.update(torch.zeros(2, 1, C, 9, 16), torch.zeros(2, C, 9, 16), torch.zeros(()), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        h.update(torch.zeros(2, 3, C, 9, 16), torch.zeros(2, C, 9, 16), torch.zeros(()), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        h.metric_handles[0].update(torch.zeros(2, C, 9, 16), torch.zeros(2, C, 9, 16), 0)


def test_the_time_quadratures():
    import makani_amd as ma
    for steps in (2, 3, 4, 5, 8):
        q = ma.Quadrature(steps - 1, 1.0 / steps, "cpu")
        assert isinstance(q.quad, ma.SimpsonQuadrature if (steps - 1) % 2 == 0 else ma.TrapezoidQuadrature)
        x = torch.randn(steps, 4)
        want = (x.double() * mh.time_weights(steps).unsqueeze(1)).sum(0)
        assert ref.mismatch(q(x, dim=0), want) < 1e-6
    with pytest.raises(NotImplementedError):
        ma.SimpsonQuadrature(3, 0.25, "cpu")


class Fp32Formula(mh.Handler):
    """the reference's sequence of operations in plain fp32 torch on the CPU"""

    def value(self, name, idx, f, t, w):
        f, t, q = f.float(), t.float(), self.q.float()
        E = f.shape[1]
        wt = (q * w.float()) if w is not None else q.expand(t.shape)
        sc = self.scale[idx].float()
        mean = torch.sum(f, dim=1) / float(E)
        quad = lambda g: torch.sum(g * wt, dim=(-2, -1))          # noqa: E731
        if name == "L1":
            return quad(torch.abs(mean - t)).sum(0)
        if name == "RMSE":
            return torch.sqrt(quad(torch.square(mean - t)).sum(0)) * sc
        if name == "ACC":
            b = self.clim[0, idx].float() if self.clim is not None else 0.0
            xa, ya = mean - b, t - b
            return (quad(xa * ya) / (torch.sqrt(quad(xa * xa) * quad(ya * ya)) + 1e-8)).sum(0)
        if name == "CRPS":
            return quad(_crps_ref.point_score(f, t, "skillspread")).sum(0) * sc
        if name == "Rank Histogram":
            fs, _ = torch.sort(torch.moveaxis(f.flatten(3), 1, -1), dim=-1, descending=False, stable=True)
            ins = torch.searchsorted(fs.contiguous(), t.flatten(2).unsqueeze(-1).contiguous(), side="right").squeeze(-1)
            return torch.sum(F.one_hot(ins, num_classes=E + 1).to(torch.float32) * wt.flatten(2).unsqueeze(-1), dim=2).sum(0)
        var = quad(torch.sum(torch.square(mean.unsqueeze(1) - f), dim=1)) / float(E - 1)
        if name == "Spread":
            return torch.sqrt(var).sum(0) * sc
        return torch.sqrt(var / torch.clamp(quad(torch.square(mean - t)) - var / float(E), min=1e-6)).sum(0)


@pytest.mark.parametrize("key", cases.CASES + ["clamp"], ids=lambda k: k if isinstance(k, str) else cases.case_id(k))
def test_inputs_let_the_fp32_formula_meet_the_gpu_tolerance(key):
    clamp = key == "clamp"
    key = cases.CLAMP_KEY if clamp else key
    want, got = cases.restatement(key, clamp), cases.restatement(key, clamp, Fp32Formula)
    worst, bins, zeros = cases.compare(got.curve, got.counter, want, cases.CLAMP_HANDLES if clamp else None)
    print(f"{'clamp' if clamp else cases.case_id(key)}: fp32 torch formula vs fp64 restatement, curves {worst:.2e} bins {bins:.2e}")
    assert worst < TOL_GPU and bins < TOL_GPU and zeros
    if clamp:          # the clamp of SSR is active on every sample: the value is sqrt(spread / eps)
        for call in range(cases.STEPS):
            prd, tar, _ = cases.call_inputs(key, call, True)
            idx = [cases.NAMES.index(c) for c in cases.LISTS["ssr_var_names"]]
            skill, ss, _ = ref.ens_sums(prd[:, :, idx], tar[:, idx], want.q)
            assert float((skill - ss / (key[1] - 1) / key[1]).max()) < -0.05
    elif key[1] > 1:
        prd, tar, _ = cases.call_inputs(key, 0)
        idx = [cases.NAMES.index(c) for c in cases.LISTS["ssr_var_names"]]
        skill, ss, _ = ref.ens_sums(prd[:, :, idx], tar[:, idx], want.q)
        assert float((skill - ss / (key[1] - 1) / key[1]).min()) > 0.1          # well above eps = 1e-6
    if not clamp and key[4] is not None:          # NaN targets: that handle counts quadrature weight, a NaN-free handle counts samples
        exact = float(cases.B * cases.PASSES)
        for name, ch, _ in want.handles:
            if key[4] in ch and not key[3]:
                i = ch.index(key[4])
                assert float(want.counter[name][0, i].reshape(-1)[0]) < exact - 0.1
            elif not key[3]:
                assert bool((want.counter[name] == exact).all())
