"""CPU tests of how the input noise is wired: InputNoise.from_params (the restatement of Preprocessor2D.__init__,
makani/models/preprocessor.py:149-232), noise_seed_reflect(share_over_model=True), the order in which the rollout wrappers
advance and read the noise (makani/models/stepper.py:76-101, 226-315) over a stub process, and the host-side argument checks of
mk_noise_update_shard."""
import ctypes

import pytest
import torch

from makani_amd.stepper import MultiStepWrapper, SingleStepWrapper


class _Params(dict):
    __getattr__ = dict.__getitem__


NAMES = ["u10m", "v10m", "t2m", "z500"]


def _params(noise, **kw):
    base = dict(input_noise=noise, channel_names=NAMES, img_shape_x_resampled=9, img_shape_y_resampled=16,
                model_grid_type="legendre-gauss", n_history=1, batch_size=2, dt=2, dhours=6)
    base.update(kw)
    return _Params(base)


# ---- 12. InputNoise.from_params ------------------------------------------------------------------------------------------------
def test_from_params_builds_the_diffusion_stage_with_the_references_defaults():
    import makani_amd as ma
    stage = ma.InputNoise.from_params(_params({"type": "diffusion", "n_channels": 3, "sigma": 2.0, "kT": [0.1, 0.2, 0.3], "lmax": 6}))
    m = stage.input_noise
    assert isinstance(stage, ma.InputNoise) and isinstance(m, ma.DiffusionNoiseS2)
    assert (stage.input_noise_mode, stage.perturb_channels, stage.n_history) == ("concatenate", None, 1)
    assert (m.nlat, m.nlon, m.num_channels, m.num_time_steps, m.lmax, m.sigma, m.kT) == (9, 16, 3, 2, 6, 2.0, [0.1, 0.2, 0.3])
    assert m.lambd == 2 * 6 / 6.0 and m.isht.grid == "legendre-gauss" and not m.learnable and not m.reflect
    assert tuple(m.state.shape) == (2, 2, 3, 6, 6, 2) and m.rng.tolist() == [333, 0]
    m = ma.InputNoise.from_params(_params({"type": "diffusion", "lambd": 0.25, "centered": True, "learnable": True}, n_history=0)).input_noise
    assert (m.num_channels, m.num_time_steps, m.lambd, m.learnable, m.reflect) == (1, 1, 0.25, True, True)
    assert m.kT == 0.5 * (100 / 6370) ** 2 and m.sigma == 1.0 and m.lmax == 9 and m.rng.tolist() == [333, 0]


def test_from_params_looks_the_perturbed_channels_up_by_name():
    import makani_amd as ma
    p = _params({"type": "white", "mode": "perturb", "perturb_channels": ["z500", "u10m"], "alpha": 2.0, "sigma": 3.0})
    del p["dt"], p["dhours"]                                                     # only the diffusion default reads them
    stage = ma.InputNoise.from_params(p)
    m = stage.input_noise
    assert isinstance(m, ma.IsotropicGaussianRandomFieldS2) and (m.alpha, m.sigma, m.num_channels, m.num_time_steps) == (2.0, 3.0, 2, 2)
    assert (stage.input_noise_mode, stage.perturb_channels) == ("perturb", [3, 0])
    stage = ma.InputNoise.from_params(_params({"type": "dummy", "mode": "perturb"}))
    assert stage.perturb_channels == [0, 1, 2, 3] and isinstance(stage.input_noise, ma.DummyNoiseS2)
    assert tuple(stage.input_noise.state.shape) == (2, 2, 4, 9, 16) and stage.input_noise.mode == "constant_zero"
    assert tuple(ma.InputNoise.from_params(_params({"type": "dummy"})).input_noise.state.shape) == (2, 2, 1, 9, 16)
    with pytest.raises(ValueError, match="is not in list"):
        ma.InputNoise.from_params(_params({"type": "white", "mode": "perturb", "perturb_channels": ["q850"]}))


def test_from_params_error_messages():
    import makani_amd as ma
    with pytest.raises(ValueError, match="please specify an input noise type"):
        ma.InputNoise.from_params(_params({"mode": "concatenate"}))
    with pytest.raises(NotImplementedError, match="input noise mode replace not supported"):
        ma.InputNoise.from_params(_params({"type": "white", "mode": "replace"}))
    with pytest.raises(NotImplementedError, match="noise type pink not supported"):
        ma.InputNoise.from_params(_params({"type": "pink"}))
    with pytest.raises(ValueError, match="input_noise is not set"):
        ma.InputNoise.from_params(_params(None))


# ---- 13. the seed shared over the model ranks --------------------------------------------------------------------------------
def test_share_over_model_takes_the_model_rank_out_of_the_seed(monkeypatch):
    import makani_amd as ma
    from makani_amd import comm
    assert ma.noise_seed_reflect(False, share_over_model=True) == (333, False)
    for name, size, rank in (("model", 4, 3), ("data", 6, 5), ("ensemble", 2, 1), ("batch", 3, 2)):
        monkeypatch.setitem(comm._GROUPS, name, (None, size, rank))
    assert ma.noise_seed_reflect(False, seed_offset=1, share_over_model=True) == (333 + 1 + 0 + 4 * 5, False)
    assert ma.noise_seed_reflect(False, seed_offset=1) == (333 + 1 + 3 + 4 * 5, False)
    assert ma.noise_seed_reflect(True, share_over_model=True) == (333 + 0 + 4 * 0 + 4 * 2 * 2, False)
    assert ma.noise_seed_reflect(True) == (333 + 3 + 4 * 0 + 4 * 2 * 2, False)
    with pytest.raises(TypeError):
        ma.noise_seed_reflect(False, 0, True)                                    # keyword only
    cfg = {"type": "white"}
    assert ma.InputNoise.from_params(_params(cfg)).input_noise.rng.tolist() == [333 + 4 * 5, 0]
    assert ma.InputNoise.from_params(_params(cfg), share_over_model=False).input_noise.rng.tolist() == [333 + 3 + 4 * 5, 0]


# ---- 14. the order of calls in the wrappers ------------------------------------------------------------------------------------
B, C, NC, H, W = 2, 3, 2, 2, 4


class _StubProcess(torch.nn.Module):
    """records update(replace_state, batch_size) and forward; the field is a constant that counts the updates"""

    def __init__(self, log, T):
        super().__init__()
        self.register_buffer("state", torch.zeros(B, T, NC, 1, 1, 2), persistent=False)
        self.log, self.T, self.updates = log, T, 0

    def is_stateful(self):
        return True

    def update(self, replace_state=False, batch_size=None):
        self.log.append(("update", replace_state, batch_size))
        self.updates += 1
        if batch_size is not None and batch_size != self.state.shape[0]:
            self.state = torch.zeros(batch_size, *self.state.shape[1:])

    def forward(self):
        self.log.append("forward")
        return torch.full((self.state.shape[0], self.T, NC, H, W), 100.0 * self.updates)


class _Net(torch.nn.Module):
    """newest time level + 1; keeps what it was given"""

    def __init__(self, log, T):
        super().__init__()
        self.log, self.T, self.seen = log, T, []

    def forward(self, x):
        self.log.append("net")
        x = x.reshape(x.shape[0], self.T, -1, H, W)
        self.seen.append(x)
        return x[:, -1, :C] + 1.0


def _wrapped(n_history, n_future=2):
    import makani_amd as ma
    log = []
    stub, net = _StubProcess(log, n_history + 1), _Net(log, n_history + 1)
    stage = ma.InputNoise(stub, n_history=n_history)
    return log, stub, net, MultiStepWrapper(net, n_future=n_future, n_history=n_history, input_noise=stage)


def test_training_rollout_updates_once_before_the_loop_and_between_steps():
    log, stub, net, wrap = _wrapped(n_history=1)
    wrap.train()
    x = torch.randn(B, 2 * C, H, W)
    y = wrap(x, update_state=True, replace_state=True)
    step = ["forward", "net"]
    assert log == [("update", True, None)] + step + [("update", False, None)] + step + [("update", False, None)] + step
    new = x[:, C:]
    p1 = new + 1.0
    p2 = p1 + 1.0
    assert torch.equal(y, torch.cat([p1, p2, p2 + 1.0], dim=1))
    # the network saw the noise of that step behind every time level, the history window itself stayed un-noised
    windows = [x, torch.cat([new, p1], 1), torch.cat([p1, p2], 1)]
    for k, (seen, window) in enumerate(zip(net.seen, windows)):
        assert tuple(seen.shape) == (B, 2, C + NC, H, W)
        assert torch.equal(seen[:, :, :C], window.reshape(B, 2, C, H, W)) and bool((seen[:, :, C:] == 100.0 * (k + 1)).all())
    del log[:]
    wrap(x, update_state=True, replace_state=False)
    assert log[0] == ("update", False, None) and len(log) == 9
    del log[:]
    wrap(x, update_state=False)
    assert log == step + [("update", False, None)] + step + [("update", False, None)] + step


def test_evaluation_sizes_the_state_to_the_batch_and_takes_one_step():
    log, stub, net, wrap = _wrapped(n_history=0)
    wrap.eval()
    x = torch.randn(5, C, H, W)
    y = wrap(x, update_state=True, replace_state=True)
    assert log == [("update", True, 5), "forward", "net"] and stub.state.shape[0] == 5
    assert torch.equal(y, x + 1) and tuple(net.seen[0].shape) == (5, 1, C + NC, H, W)
    del log[:]
    wrap(x, update_state=False)
    assert log == ["forward", "net"]
    with pytest.raises(RuntimeError, match="refusing to resize"):
        wrap(x[:3], replace_state=False)


def test_single_step_wrapper_carries_the_noise_into_both_entries():
    import makani_amd as ma
    log = []
    stub, net = _StubProcess(log, 1), _Net(log, 1)
    net.encode_process = lambda x: x * 2.0
    single = SingleStepWrapper(net, input_noise=ma.InputNoise(stub))
    x = torch.randn(B, C, H, W)
    assert torch.equal(single(x), x + 1) and log == [("update", True, B), "forward", "net"]
    del log[:]
    z = single.encode_process(x, update_state=True, replace_state=False)
    assert log == [("update", False, B), "forward"] and tuple(z.shape) == (B, C + NC, H, W) and torch.equal(z[:, :C], 2 * x)
    del log[:]
    single(x, update_state=False)
    assert log == ["forward", "net"]


def test_wrapper_refuses_a_noise_stage_of_another_history_length():
    import makani_amd as ma
    stage = ma.InputNoise(_StubProcess([], 1), n_history=0)
    with pytest.raises(ValueError, match="n_history"):
        MultiStepWrapper(torch.nn.Identity(), n_future=1, n_history=1, input_noise=stage)


# ---- 15. from_params of the wrapper still refuses params.input_noise -----------------------------------------------------------
def test_wrapper_from_params_names_the_keyword_when_it_refuses_input_noise():
    p = _Params(n_future=1, n_history=0, history_normalization_mode="none", input_noise={"type": "white"})
    with pytest.raises(NotImplementedError, match=r"InputNoise\.from_params.*input_noise= keyword"):
        MultiStepWrapper.from_params(p, lambda: torch.nn.Identity())


# ---- the host-side checks of the shard entry -----------------------------------------------------------------------------------
def test_library_validates_shard_arguments_on_the_host():
    from makani_amd import _lib
    L, p, null = _lib.lib(), ctypes.c_void_p(64), ctypes.c_void_p(0)

    def call(state=p, xi=null, sigma=p, phi=p, rng=p, mode=1, dims=(1, 1, 1, 4, 8), box=(0, 4, 0, 8)):
        return L.mk_noise_update_shard(state, xi, sigma, phi, rng, mode, *dims, *box, 0, None)

    for kw, msg in ((dict(state=null), b"null state"), (dict(rng=null), b"null rng"), (dict(sigma=null), b"null sigma"),
                    (dict(phi=null), b"null sigma / phi"), (dict(mode=3), b"unknown mode 3"), (dict(dims=(1, 0, 1, 4, 8)), b"T >= 1"),
                    (dict(dims=(0, 1, 1, 4, 8)), b"bad shape"), (dict(box=(2, 3, 0, 8)), b"rows [2, 2 + 3) leave the global [0, 4)"),
                    (dict(box=(-1, 1, 0, 8)), b"rows [-1"), (dict(box=(0, 0, 0, 8)), b"rows [0, 0 + 0)"),
                    (dict(box=(0, 4, 6, 4)), b"floats [6, 6 + 4) leave the global row [0, 8)"), (dict(box=(0, 4, -2, 2)), b"floats [-2"),
                    (dict(box=(0, 4, 8, 0)), b"floats [8, 8 + 0)"), (dict(box=(0, 4, 0, 1 << 30)), b"floats"),
                    (dict(dims=(1, 1, 1 << 15, 1 << 8, 1 << 8), box=(0, 1, 0, 2)), b"2^31")):
        assert call(**kw) < 0 and msg in L.mk_last_error(), (kw, L.mk_last_error())
