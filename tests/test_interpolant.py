"""The stochastic-interpolant stepper on the CPU: the fp64 restatement tests/_interp_ref.py against the arrays recorded from the
reference's own class (tests/golden/interpolant.npz, tools/make_interpolant_golden.py), the closed-form step coefficients of
``makani_amd.interpolant`` against the generic formula, and the constructor / ``from_params`` contract.  The kernels themselves are
compared with the restatement in tests/test_gpu_interpolant.py."""
import pytest
import torch

import _interp_ref as ref
from _preproc_ref import seeded
from conftest import load_golden

CASES = ref.load_cases(load_golden("interpolant.npz"))
NAMES = sorted(CASES)
TOL = 1e-12          # of the largest magnitude: a few dozen roundings of 1.1e-16 at the well-conditioned s in {1/3, 2/3}


def _stub(c):
    m = c["meta"]
    cin = 2 * m["C"] + m["U"] + m["St"] + (0 if m["time_aware"] else 1)
    w = (m["net_scale"][0] * seeded((m["C"], cin, 1, 1), m["seeds"]["net"])).float()
    b = (m["net_scale"][1] * seeded((m["C"],), m["seeds"]["net"] + 1)).float()
    return w, b


def test_the_fixture_holds_every_case_of_the_issue():
    metas = [c["meta"] for c in CASES.values()]
    combos = {(m["eps"], m["foellmer"], m["antithetic"]) for m in metas if not m["time_aware"]}
    assert combos == {(e, f, a) for e in (1.0, 0.7) for f in (False, True) for a in (False, True)}
    assert any(m["U"] == 2 and m["St"] == 2 for m in metas) and any(m["U"] == 0 and m["St"] == 0 for m in metas)
    assert sum(m["time_aware"] for m in metas) == 1
    assert all(m["sampler_B"] == 1 for m in metas if m["St"])


@pytest.mark.parametrize("case", NAMES)
def test_restatement_equals_the_reference_in_float64(case):
    c = CASES[case]
    m = c["meta"]
    x0, x1, xu, static = ref.case_inputs(c)
    C = m["C"]
    assert (static is not None) == bool(m["St"])
    assert c["s"].shape == (m["B"], m["n_samples"] * (2 if m["antithetic"] else 1))
    if m["antithetic"]:
        assert torch.equal(c["s"], torch.cat([c["s_draw"], 1.0 - c["s_draw"]], dim=1))
    X, D = ref.assemble(x0, x1, c["z"], c["s"], None if xu is None else xu[:, 0], None if static is None else static[0], m["eps"],
                        has_s=not m["time_aware"])
    for got, want in ((X[:, C:2 * C], c["x64"]), (D, c["drift64"])):
        assert want.dtype == torch.float64 and float((got - want).abs().max()) <= TOL * float(want.abs().max())
    w, b = _stub(c)
    net = ref.stub(w, b)
    if "pred64" in c:
        pred = net(X)
        assert float((pred - c["pred64"]).abs().max()) <= TOL * float(c["pred64"].abs().max())
    n = m["sampler_B"]
    for steps in m["n_steps"]:
        y = ref.sampler(net, x0[:n], None if xu is None else xu[:n, 0], None if static is None else static[0], list(c[f"noise_n{steps}"]),
                        steps, m["eps"], m["foellmer"], time_aware=m["time_aware"])
        want = c[f"y64_n{steps}"]
        assert float((y - want).abs().max()) <= TOL * float(want.abs().max()), (case, steps)


@pytest.mark.parametrize("eps", [1.0, 0.7])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 7])
def test_closed_form_step_coefficients_equal_the_generic_formula(eps, n_steps):
    from makani_amd.interpolant import step_coefficients
    st = torch.linspace(0, 1, n_steps + 1, dtype=torch.float32)
    ds = (st[1:] - st[:-1]).double().tolist()
    st = st.double().tolist()
    for foellmer in (False, True):
        for i in range(n_steps):
            got = step_coefficients(st[i], ds[i], eps, foellmer=foellmer, first=i == 0)
            want = ref.generic_coefficients(st[i], ds[i], eps, foellmer, i == 0)
            for g, w_ in zip(got, want):
                assert abs(g - w_) <= 1e-13 * max(1.0, abs(w_)), (eps, n_steps, foellmer, i, got, want)
    with pytest.raises(ValueError, match="singular"):
        step_coefficients(0.0, 0.5, eps, foellmer=True, first=False)


def test_tensor_functions_follow_the_restatement():
    import makani_amd as ma
    w = ma.StochasticInterpolantWrapper(torch.nn.Identity(), ma.Preprocessor2D(img_shape=(9, 16)),
                                        ma.IsotropicGaussianRandomFieldS2((9, 16), 2, 3), n_pred_chans=3, noise_epsilon=0.7)
    s = torch.tensor([0.0, 0.25, 2.0 / 3.0], dtype=torch.float64)
    for f in (False, True):
        assert torch.allclose(w.gsq_fn(s, foellmer=f), ref.gsq(s, 0.7, f), rtol=1e-14, atol=0)
    x, x0, b = (seeded((3, 2), k) for k in (1, 2, 3))
    si = s[1:].reshape(1, 2)
    assert torch.allclose(w.dlog_rho(x[1:].T, x0[1:].T, b[1:].T, si), ref.score(x[1:].T, x0[1:].T, b[1:].T, si, 0.7), rtol=1e-14)
    a, t, z = (seeded((2, 3, 4, 5), k).unsqueeze(1) for k in (4, 5, 6))
    sb = torch.tensor([[0.0, 0.3, 1.0], [0.5, 0.9, 0.1]], dtype=torch.float64)
    inter, drift = w.stochastic_path(a, t, z, sb)
    wi, wd = ref.path(a[:, 0], t[:, 0], z[:, 0], sb, 0.7)
    assert torch.allclose(inter.flatten(0, 1), wi, rtol=1e-14, atol=1e-15) and torch.allclose(drift.flatten(0, 1), wd, rtol=1e-14, atol=1e-15)
    assert w.stochastic_path(a, t, z, sb, return_derivative=False).shape == inter.shape


class _Params(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _params(**over):
    p = _Params(img_shape_x=9, img_shape_y=16, img_shape_x_resampled=9, img_shape_y_resampled=16, img_crop_shape_x=9, img_crop_shape_y=16,
                n_history=0, n_future=0, N_in_predicted_channels=3, N_out_channels=3, N_static_channels=0, N_dynamic_channels=2, batch_size=2,
                data_grid_type="equiangular", model_grid_type="equiangular")
    p.update(over)
    return p


def test_from_params_builds_the_reference_layout_and_raises_its_errors():
    import makani_amd as ma
    seen = {}

    def handle(inp_chans):
        seen["inp_chans"] = inp_chans
        return torch.nn.Conv2d(inp_chans, 3, 1)

    w = ma.StochasticInterpolantWrapper.from_params(_params(), handle, noise_epsilon=0.7, use_foellmer=True, antithetic_sampling=True)
    assert seen["inp_chans"] == 2 * 3 + 0 + 2 + 1 and isinstance(w.model, ma.InterpolationWrapper)
    assert isinstance(w.preprocessor, ma.Preprocessor2D) and isinstance(w.noise_module, ma.IsotropicGaussianRandomFieldS2)
    nm = w.noise_module
    assert (nm.nlat, nm.nlon, nm.num_channels, nm.num_time_steps, nm.sigma, nm.alpha) == (9, 16, 3, 1, 1.0, 0.0)
    assert tuple(nm.state.shape[:3]) == (2, 1, 3) and nm.rng.tolist() == [333, 0]
    assert (w.noise_epsilon, w.use_foellmer, w.antithetic_sampling, w.time_aware) == (0.7, True, True, False)
    assert w.get_internal_rng(gpu=False) is w.rng_cpu and w.rng_cpu.initial_seed() == 333 + 333
    w = ma.StochasticInterpolantWrapper.from_params(_params(time_aware=True, N_static_channels=4), handle, seed=5)
    assert seen["inp_chans"] == 2 * 3 + 4 + 2 and isinstance(w.model, ma.TimeAwareInterpolationWrapper) and w.time_aware
    assert w.noise_module.rng.tolist() == [5, 0] and w.rng_cpu.initial_seed() == 5 + 333
    with pytest.raises(ValueError, match=r"this model currently does not support history, expected n_history == 0 but got 2"):
        ma.StochasticInterpolantWrapper.from_params(_params(n_history=2), handle)
    with pytest.raises(ValueError, match=r"this model currently does not support future steps, expected n_future == 0 but got 1"):
        ma.StochasticInterpolantWrapper.from_params(_params(n_future=1), handle)
    with pytest.raises(ValueError, match=r"expected N_in_predicted_channels \(3\) to match N_out_channels \(4\)"):
        ma.StochasticInterpolantWrapper.from_params(_params(N_out_channels=4), handle)


def test_constructor_contract():
    import makani_amd as ma
    pre, noise = ma.Preprocessor2D(img_shape=(9, 16)), ma.IsotropicGaussianRandomFieldS2((9, 16), 2, 3)
    net = torch.nn.Conv2d(7, 3, 1)
    w = ma.StochasticInterpolantWrapper(net, pre, noise, n_pred_chans=3)
    assert isinstance(w.model, ma.InterpolationWrapper) and w.model.model is net and w.input_dtype is None
    inner = ma.TimeAwareInterpolationWrapper(lambda inp_chans: torch.nn.Conv2d(inp_chans, 3, 1), 3, 0, 0)
    assert ma.StochasticInterpolantWrapper(inner, pre, noise, n_pred_chans=3, time_aware=True).model is inner
    with pytest.raises(TypeError, match="time_aware"):
        ma.StochasticInterpolantWrapper(inner, pre, noise, n_pred_chans=3)
    with pytest.raises(ValueError, match="does not support history"):
        ma.StochasticInterpolantWrapper(net, ma.Preprocessor2D(img_shape=(9, 16), n_history=1), noise, n_pred_chans=3)
    with pytest.raises(TypeError, match="input_dtype"):
        ma.StochasticInterpolantWrapper(net, pre, noise, n_pred_chans=3, input_dtype=torch.float16)
    # the plain wrappers compose by hand as in the reference
    plain = ma.InterpolationWrapper(lambda inp_chans: torch.nn.Conv2d(inp_chans, 3, 1), 3, 2, 1)
    assert plain.model.in_channels == 3 * 2 + 2 + 1 + 1
    x0, x, xu, st, s = torch.randn(2, 3, 4, 5), torch.randn(2, 3, 4, 5), torch.randn(2, 1, 4, 5), torch.randn(2, 2, 4, 5), torch.rand(2)
    want = plain.model(torch.cat([x0, x, xu, st, s.reshape(2, 1, 1, 1).expand(2, 1, 4, 5)], dim=1))
    assert torch.equal(plain(x0, x, xu, st, s), want)


def test_exports():
    import makani_amd as ma
    for name in ("InterpolationWrapper", "TimeAwareInterpolationWrapper", "StochasticInterpolantWrapper"):
        assert name in ma.__all__ and hasattr(ma, name)


def test_cpu_tensors_raise():
    import makani_amd as ma
    w = ma.StochasticInterpolantWrapper(torch.nn.Conv2d(7, 3, 1), ma.Preprocessor2D(img_shape=(9, 16)),
                                        ma.IsotropicGaussianRandomFieldS2((9, 16), 2, 3), n_pred_chans=3)
    x = torch.randn(2, 3, 9, 16)
    for mode in (True, False):
        w.train(mode)
        with pytest.raises(RuntimeError, match="GPU"):
            w(x, x)
