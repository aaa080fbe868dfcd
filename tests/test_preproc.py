"""``Preprocessor2D`` without a GPU: the fp64 restatement (tests/_preproc_ref.py) against tests/golden/preproc.npz, recorded by
tools/make_preproc_golden.py from the reference's own class; construction, ``from_params``, the host-side methods, the wrappers'
``preprocessor=`` keyword and the argument validation of the C ABI.

Gate: relative L2 <= 1e-5 on every stored array — the fixtures are the reference's fp32 arithmetic on well-conditioned inputs
(|mu| / sigma <= 3), the restatement is fp64."""
import ctypes
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _preproc_ref as ref          # noqa: E402
from conftest import load_golden          # noqa: E402

TOL = 1e-5


class Params(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _cases():
    g = load_golden("preproc.npz")
    names = sorted({k.split("/")[0] for k in g.files})
    out = {}
    for name in names:
        c = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
        c["meta"] = json.loads(str(c["meta"]))
        out[name] = c
    return out


CASES = _cases()


def _inputs(c):
    m, sd = c["meta"], c["meta"]["seeds"]
    H, W = m["img_shape"]
    T = m["n_history"] + 1
    win = ref.seeded_field((m["B"], T, m["C"], H, W), sd["win"]).flatten(1, 2)
    xz = ref.seeded_field((m["B"], T, m["U"], H, W), sd["xz"])
    yz = ref.seeded_field((m["B"], 2, m["U"], H, W), sd["yz"])
    yn = ref.seeded((m["B"], m["C"], H, W), sd["yn"]).float().double()
    return win, xz, yz, yn


def test_the_fixture_holds_the_twelve_cases():
    assert len(CASES) == 12
    assert {(c["meta"]["mode"], c["meta"]["n_history"], c["meta"]["rich"]) for c in CASES.values()} == \
        {(m, h, r) for m in ("none", "mean", "exponential") for h in (0, 2) for r in (False, True)}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "preproc.npz")) < 2 ** 20


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_reference_fixture(name):
    c = CASES[name]
    m, sd = c["meta"], c["meta"]["seeds"]
    H, W = m["img_shape"]
    T, mode = m["n_history"] + 1, m["mode"]
    win, xz, yz, yn = _inputs(c)
    win.requires_grad_(True)
    yn.requires_grad_(True)
    static = torch.from_numpy(c["static"])[0].double() if m["rich"] else None
    bias = torch.from_numpy(c["bias"])[0].double() if m["rich"] else None
    q, wt = ref.quad_weights(H, W), (None if mode == "none" else ref.time_weights(mode, m["n_history"], 0.5))
    out, mu, sigma = ref.assemble(win, xz, None, static, T, mode, q, wt)
    y = ref.finish(yn, bias, mu, sigma)
    r1, r2 = ref.seeded(out.shape, sd["r1"]).float().double(), ref.seeded(y.shape, sd["r2"]).float().double()
    gwin, gyn = torch.autograd.grad((out * r1).sum() + (y * r2).sum(), [win, yn])
    # one rollout step: the window slides, and the cached unpredicted input takes level 0 of the target's
    nxt = ref.append_history(win.detach(), torch.from_numpy(c["y"]).double(), T)
    unp = ref.slide(xz, yz, 0)
    errs = {"out": ref.rel(out, torch.from_numpy(c["out"])), "y": ref.rel(y, torch.from_numpy(c["y"])),
            "gwin": ref.rel(gwin, torch.from_numpy(c["gwin"])), "gyn": ref.rel(gyn, torch.from_numpy(c["gyn"])),
            "next_window": ref.rel(nxt, torch.from_numpy(c["next_window"])) if T > 1 else 0.0,
            "next_unpredicted": ref.rel(unp, torch.from_numpy(c["next_unpredicted"]))}
    if mode == "none":
        assert tuple(c["history_mean"].shape) == (1, 1, 1, 1) and c["history_mean"].item() == 0.0 and c["history_std"].item() == 1.0
    else:
        assert tuple(c["history_mean"].shape) == (m["B"], m["C"] + m["U"], 1, 1)
        errs["history_mean"] = ref.rel(mu, torch.from_numpy(c["history_mean"]).reshape(mu.shape))
        errs["history_std"] = ref.rel(sigma, torch.from_numpy(c["history_std"]).reshape(sigma.shape))
        assert float((mu.abs() / sigma).max().detach()) <= 3.0
    print(name + ": " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL, errs


# ---- construction ----------------------------------------------------------------------------------------------------------
def _params(c, **extra):
    p = Params(c["meta"]["params"])
    p.update(batch_size=c["meta"]["B"], **extra)
    return p


def test_constructor_buffers_and_shapes():
    import makani_amd as ma
    pre = ma.Preprocessor2D(img_shape=(9, 16), n_history=2, history_normalization_mode="exponential", history_normalization_decay=0.5,
                            static_features=torch.zeros(1, 4, 9, 16), bias_correction=torch.zeros(1, 3, 9, 16))
    w = ref.time_weights("exponential", 2, 0.5)
    assert tuple(pre.history_normalization_weights.shape) == (1, 3, 1, 1, 1)
    assert ref.rel(pre.history_normalization_weights.reshape(3), w) < 1e-6 and ref.rel(pre.history_time_weights, w) < 1e-6
    assert tuple(pre.quadrature.quad_weight.shape) == (1, 1, 9, 16)
    assert ref.rel(pre.quadrature.quad_weight[0, 0], ref.quad_weights(9, 16)) < 1e-6
    assert pre.do_add_static_features and tuple(pre.get_static_features().shape) == (1, 4, 9, 16)
    assert tuple(pre.bias_correction.shape) == (1, 3, 9, 16)
    assert pre.history_mean is None and pre.history_std is None and pre.noise_stage is None and not pre.spatial_distributed
    assert not pre.state_dict()          # every buffer is non-persistent, as in the reference
    mean = ma.Preprocessor2D(img_shape=(9, 16), n_history=2, history_normalization_mode="mean")
    assert tuple(mean.history_normalization_weights.shape) == (1, 1, 1, 1, 1) and float(mean.history_normalization_weights) == pytest.approx(1 / 3)
    assert mean.history_time_weights.tolist() == pytest.approx([1 / 3] * 3)
    none = ma.Preprocessor2D(img_shape=(9, 16), n_history=2)
    assert none.history_normalization_weights.tolist() == [1.0, 1.0, 1.0] and not hasattr(none, "quadrature")
    assert not none.do_add_static_features and none.get_static_features() is None and not hasattr(none, "bias_correction")
    x = torch.zeros(2, 6, 9, 16)
    assert none.add_static_features(x) is x and none.correct_bias(x) is x and none.finish(x) is x and none.assemble(x) is x
    assert none.history_normalize(x) is x and none.history_denormalize(x, target=True) is x


def test_refusals_of_the_constructor():
    import makani_amd as ma
    with pytest.raises(NotImplementedError, match="timediff.*only works for B in"):
        ma.Preprocessor2D(img_shape=(9, 16), history_normalization_mode="timediff")
    with pytest.raises(NotImplementedError, match="'max'.*un-normalised weights"):
        ma.Preprocessor2D(img_shape=(9, 16), history_normalization_mode="max")
    with pytest.raises(ValueError, match="needs history_normalization_decay"):
        ma.Preprocessor2D(img_shape=(9, 16), history_normalization_mode="exponential")
    with pytest.raises(ValueError, match=r"expected \(1, S, H, W\)"):
        ma.Preprocessor2D(img_shape=(9, 16), static_features=torch.zeros(4, 9, 16))
    with pytest.raises(ValueError, match=r"expected \(1, C_out, H, W\)"):
        ma.Preprocessor2D(img_shape=(9, 16), bias_correction=torch.zeros(2, 3, 9, 16))
    noise = ma.InputNoise(ma.DummyNoiseS2((9, 16), 2, 1, num_time_steps=2), n_history=1)
    with pytest.raises(ValueError, match="input_noise carries n_history = 1, the preprocessor 0"):
        ma.Preprocessor2D(img_shape=(9, 16), input_noise=noise)


@pytest.mark.parametrize("name", ["mean_h2_rich", "none_h0_rich", "exponential_h0_rich"])
def test_from_params_builds_the_grid_planes_of_the_fixture(name):
    import makani_amd as ma
    c = CASES[name]
    static, bias = torch.from_numpy(c["static"]), torch.from_numpy(c["bias"])
    assert tuple(static.shape) == (1, 9, 9, 16)          # 2 coordinates x 2 frequencies x (sin, cos), then the orography plane
    pre = ma.Preprocessor2D.from_params(_params(c), static_features=static[:, 8:], bias_correction=bias)
    assert pre.n_history == c["meta"]["n_history"] and pre.history_normalization_mode == c["meta"]["mode"]
    assert tuple(pre.static_features.shape) == (1, 9, 9, 16) and torch.equal(pre.static_features[:, 8:], static[:, 8:])
    diff = (pre.static_features[:, :8] - static[:, :8]).abs().max().item()
    print(f"{name}: add_grid planes, largest difference from the reference's {diff:.1e}")
    assert diff <= 2.0 ** -22          # (sin / cos of the same fp32 arguments: a few units in the last place at most)
    assert torch.equal(pre.bias_correction, bias)
    # without add_cos, one frequency, not sinusoidal
    p = _params(c, add_cos_to_grid=False, grid_num_frequencies=1)
    assert tuple(ma.Preprocessor2D.from_params(p, static[:, 8:], bias).static_features.shape) == (1, 3, 9, 16)
    p = _params(c, gridtype="linear", img_local_offset_x=2, img_local_shape_x=4)
    planes = ma.preprocessor.grid_static_features(p)
    assert tuple(planes.shape) == (1, 2, 4, 16) and planes[0, 0, :, 0].tolist() == pytest.approx([2 / 9, 3 / 9, 4 / 9, 5 / 9])
    p = _params(c, normalize_static_features=True, img_shape=(9, 16))
    planes = ma.preprocessor.grid_static_features(p).double()
    q = ref.quad_weights(9, 16)
    assert float(((planes * q).sum((-2, -1))).abs().max()) < 1e-5 and float(((planes ** 2 * q).sum((-2, -1)) - 1).abs().max()) < 1e-5


def test_from_params_refusals_name_the_keyword():
    import makani_amd as ma
    c = CASES["mean_h2_rich"]
    bias = torch.from_numpy(c["bias"])
    with pytest.raises(ValueError, match="params.add_orography is set.*static_features= keyword"):
        ma.Preprocessor2D.from_params(_params(c), bias_correction=bias)
    with pytest.raises(ValueError, match="params.bias_correction is set.*bias_correction= keyword"):
        ma.Preprocessor2D.from_params(_params(c, bias_correction="bias.h5"), static_features=torch.zeros(1, 1, 9, 16))
    with pytest.raises(ValueError, match="params.add_landmask is set.*static_features= keyword"):
        ma.Preprocessor2D.from_params(_params(CASES["mean_h2_plain"], add_landmask=True))
    with pytest.raises(NotImplementedError, match="GridConverter"):
        ma.Preprocessor2D.from_params(_params(c, lat=[0.0], lon=[0.0]), static_features=torch.zeros(1, 1, 9, 16))
    with pytest.raises(NotImplementedError, match="timediff"):
        ma.Preprocessor2D.from_params(_params(CASES["mean_h2_plain"], history_normalization_mode="timediff"))
    # the noise stage comes from InputNoise.from_params
    p = _params(CASES["mean_h2_plain"], input_noise={"type": "dummy", "n_channels": 2})
    pre = ma.Preprocessor2D.from_params(p)
    assert isinstance(pre.noise_stage, ma.InputNoise) and isinstance(pre.noise_stage.input_noise, ma.DummyNoiseS2)
    assert tuple(pre.noise_stage.input_noise.state.shape) == (2, 3, 2, 9, 16)


# ---- host-side methods -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mean_h2_plain", "none_h0_plain"])
def test_append_history_and_the_unpredicted_cache_equal_the_fixture(name):
    import makani_amd as ma
    c = CASES[name]
    nh = c["meta"]["n_history"]
    win, xz, yz, _ = _inputs(c)
    pre = ma.Preprocessor2D(img_shape=(9, 16), n_history=nh)
    pre.train()
    x, y = pre.cache_unpredicted_features("x", "y", xz.float(), yz.float())
    assert (x, y) == ("x", "y") and pre.unpredicted_inp_eval is None
    held = pre.unpredicted_inp_train
    nxt = pre.append_history(win.float(), torch.from_numpy(c["y"]), 0)
    assert torch.equal(nxt, torch.from_numpy(c["next_window"]))
    assert pre.unpredicted_inp_train is held and torch.equal(held, torch.from_numpy(c["next_unpredicted"]))
    before = held.clone()
    pre.append_history(win.float(), torch.from_numpy(c["y"]), 5)                              # beyond the cached target: untouched
    pre.append_history(win.float(), torch.from_numpy(c["y"]), 1, update_state=False)
    assert torch.equal(held, before)
    # _ensure_cached: same shape reuses the memory, another shape rebinds, None clears; the eval cache is separate
    pre.cache_unpredicted_features(None, None, xz.float(), yz.float())
    assert pre.unpredicted_inp_train is held and torch.equal(held, xz.float())
    pre.cache_unpredicted_features(None, None, xz.float()[:1], None)
    assert pre.unpredicted_inp_train is not held and pre.unpredicted_tar_train is None
    pre.eval()
    assert pre.get_unpredicted_features() == (None, None)
    pre.cache_unpredicted_features(None, None, xz.float(), yz.float())
    inpu, taru = pre.get_unpredicted_features()
    assert torch.equal(inpu, xz.float()) and inpu is not pre.unpredicted_inp_eval and torch.equal(taru, yz.float())
    assert tuple(pre.unpredicted_inp_train.shape)[0] == 1


def test_history_layout_and_statistics_checks():
    import makani_amd as ma
    pre = ma.Preprocessor2D(img_shape=(9, 16), n_history=2, history_normalization_mode="mean", static_features=torch.ones(1, 2, 9, 16))
    x = torch.arange(2 * 6 * 9 * 16, dtype=torch.float32).reshape(2, 6, 9, 16)
    x5 = pre.expand_history(x, 3)
    assert tuple(x5.shape) == (2, 3, 2, 9, 16) and pre.expand_history(x5, 3) is x5 and torch.equal(pre.flatten_history(x5), x)
    with pytest.raises(RuntimeError, match="channel dim 6 is not divisible by nhist=4"):
        pre.expand_history(x, 4)
    assert tuple(pre.remove_static_features(torch.zeros(2, 8, 9, 16)).shape) == (2, 6, 9, 16)
    with pytest.raises(RuntimeError, match="history_normalize: history_mean / history_std are None. Call history_compute_stats"):
        pre.history_normalize(x)
    with pytest.raises(RuntimeError, match="history_denormalize: history_mean / history_std are None"):
        pre.finish(x[:, :2])
    pre.history_mean, pre.history_std = torch.zeros(3, 2, 1, 1), torch.ones(3, 2, 1, 1)
    with pytest.raises(RuntimeError, match=r"batch mismatch between input \(2\) and cached history stats \(3\)"):
        pre.history_denormalize(x, target=False)
    none = ma.Preprocessor2D(img_shape=(9, 16))
    none.history_compute_stats(x)
    assert tuple(none.history_mean.shape) == (1, 1, 1, 1) and float(none.history_mean) == 0.0 and float(none.history_std) == 1.0


def test_a_cpu_tensor_raises():
    import makani_amd as ma
    pre = ma.Preprocessor2D(img_shape=(9, 16), n_history=0, history_normalization_mode="mean", static_features=torch.ones(1, 2, 9, 16),
                            bias_correction=torch.zeros(1, 3, 9, 16))
    x = torch.randn(2, 3, 9, 16)
    for call in (pre.assemble, pre.history_compute_stats, pre.add_static_features, pre.correct_bias):
        with pytest.raises(RuntimeError, match=r"GPU \(HIP\) path only"):
            call(x)


# ---- the wrappers ----------------------------------------------------------------------------------------------------------
def test_wrappers_take_the_preprocessor_keyword():
    import makani_amd as ma
    net = torch.nn.Identity()
    pre = ma.Preprocessor2D(img_shape=(9, 16), n_history=1)
    multi = ma.MultiStepWrapper(net, n_future=2, n_history=1, preprocessor=pre)
    single = ma.SingleStepWrapper(net, preprocessor=pre)
    assert multi.preprocessor is pre and single.preprocessor is pre and multi.input_noise is None
    assert ma.MultiStepWrapper(net).preprocessor is None and ma.SingleStepWrapper(net).preprocessor is None
    noise = ma.InputNoise(ma.DummyNoiseS2((9, 16), 2, 1, num_time_steps=2), n_history=1)
    for make in (lambda: ma.MultiStepWrapper(net, n_history=1, input_noise=noise, preprocessor=pre),
                 lambda: ma.SingleStepWrapper(net, input_noise=noise, preprocessor=pre)):
        with pytest.raises(ValueError, match="preprocessor= and input_noise= are both given: the noise belongs to the preprocessor"):
            make()
    with pytest.raises(ValueError, match="the preprocessor carries n_history = 1, the rollout 0"):
        ma.MultiStepWrapper(net, preprocessor=pre)


def test_identity_preprocessor_rolls_out_on_the_cpu_like_the_plain_wrapper():
    """mode "none" without features launches nothing: the preprocessor path of the wrapper is then pure torch"""
    import makani_amd as ma
    torch.manual_seed(0)
    net = torch.nn.Conv2d(4, 2, 1)
    x = torch.randn(2, 4, 9, 16)
    plain = ma.MultiStepWrapper(net, n_future=2, n_history=1)
    withp = ma.MultiStepWrapper(net, n_future=2, n_history=1, preprocessor=ma.Preprocessor2D(img_shape=(9, 16), n_history=1))
    assert torch.equal(plain(x), withp(x)) and tuple(withp(x).shape) == (2, 6, 9, 16)
    plain.eval(), withp.eval()
    assert torch.equal(plain(x), withp(x)) and tuple(withp(x).shape) == (2, 2, 9, 16)
    single = ma.SingleStepWrapper(net, preprocessor=ma.Preprocessor2D(img_shape=(9, 16), n_history=1))
    assert torch.equal(single(x), net(x))


def test_from_params_of_the_wrappers_still_refuses_the_preprocessor_keys():
    import makani_amd as ma
    for key, value in (("history_normalization_mode", "mean"), ("bias_correction", "bias.h5"), ("add_zenith", True),
                       ("add_orography", True), ("input_noise", {"type": "dummy"})):
        with pytest.raises(NotImplementedError):
            ma.MultiStepWrapper.from_params({"n_future": 1, "n_history": 0, key: value}, torch.nn.Identity)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    from makani_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    f32 = _lib.MK_F32

    def assemble(win=p, out=p, T=1, WC=3, U=0, N=0, S=0, stat=null):
        return L.mk_prep_assemble(win, f32, null, f32, null, f32, stat, f32, null, null, out, f32, 2, T, WC, U, N, S, 4, null)

    assert L.mk_prep_chunks(286) == 1 and L.mk_prep_chunks(2112) == 2 and L.mk_prep_chunks(16380) == 8
    assert L.mk_prep_chunks(721 * 1440) == 507 and L.mk_prep_chunks(10 ** 9) == 512
    for kwargs, what in ((dict(win=null), "null pointer"), (dict(out=null), "null pointer"), (dict(T=2, WC=3), "multiple of T = 2"),
                         (dict(S=-1), "S = -1"), (dict(S=2), "null pointer"), (dict(U=2), "null pointer")):
        rc = assemble(**kwargs)
        assert rc < 0 and what in L.mk_last_error().decode(), (rc, what, L.mk_last_error().decode())
    stats = L.mk_prep_stats(p, f32, null, f32, null, f32, null, p, p, p, null, p, 2, 1, 3, 0, 0, 4, null)
    assert stats < 0 and "null pointer (q, wt and ws" in L.mk_last_error().decode()
    assert L.mk_prep_stats(p, f32, null, f32, null, f32, p, p, p, p, null, p, 2, 2, 3, 0, 0, 4, null) < 0
    assert L.mk_prep_stats(p, 7, null, f32, null, f32, p, p, p, p, null, p, 2, 1, 3, 0, 0, 4, null) < 0
    assert L.mk_prep_finish(null, f32, null, null, null, p, 2, 3, 3, 4, null) < 0
    assert L.mk_prep_finish(p, f32, null, p, p, p, 2, 3, 2, 4, null) < 0 and "fewer than Cout" in L.mk_last_error().decode()
    assert L.mk_prep_bwd_sums(p, f32, p, f32, null, f32, null, f32, p, p, null, null, p, p, 2, 1, 3, 0, 0, -1, 1, 4, null) < 0
    assert L.mk_prep_bwd_sums(p, f32, p, f32, null, f32, null, f32, p, p, null, null, p, p, 2, 1, 3, 0, 0, 0, 0, 4, null) < 0
    assert L.mk_prep_bwd_sums(p, f32, p, f32, null, f32, null, f32, p, p, null, null, p, p, 2, 1, 3, 0, 1, 0, 2, 4, null) < 0
    assert L.mk_prep_bwd_apply(null, f32, p, f32, null, f32, null, f32, p, p, p, p, null, p, null, 2, 1, 3, 0, 0, 0, 4, null) < 0
    assert L.mk_prep_bwd_apply(p, f32, p, f32, null, f32, null, f32, p, p, p, p, null, null, null, 2, 1, 3, 0, 0, 0, 4, null) < 0
    assert L.mk_prep_bwd_apply(p, f32, p, f32, null, f32, null, f32, p, p, p, p, null, p, null, 2, 2, 3, 0, 0, 0, 4, null) < 0
    assert L.mk_prep_finish_bwd(p, f32, p, f32, null, p, null, p, 2, 3, 3, 4, null) < 0
    assert L.mk_prep_finish_bwd(p, f32, p, f32, null, p, p, p, 2, 3, 3, 0, null) < 0
