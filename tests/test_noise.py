"""CPU tests of the input-noise processes (makani_amd/noise.py, csrc/noise.hip): the restated generator of tests/_noise_ref.py
against the published Philox known answers and the moments of a standard normal, the modules' buffers against the fixtures
recorded from the reference's own classes (tools/make_noise_golden.py), the interface's error cases, and the InputNoise
channel logic over a stub process."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import _noise_ref as R

N = 1 << 20


# ---- the restated generator -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_restated_philox_reproduces_the_random123_known_answers(counter, key, want):
    got = " ".join(f"{int(v[0]):08x}" for v in R.philox4x32_10(counter, key))
    assert got == want


def test_uniforms_are_exact_24_bit_values_inside_their_intervals():
    x = np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32)
    u1, u2 = R.uniforms(x, x)
    assert u1.min() == 2.0 ** -24 and u1.max() == 1.0 and u2.min() == 0.0 and u2.max() == 1.0 - 2.0 ** -24
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)


@pytest.fixture(scope="module")
def normals():
    """2^20 restated normals of one time level, and the same groups one offset later (read only)"""
    z0, z1 = R.normals(333, 5, N), R.normals(333, 6, N)
    z0.setflags(write=False)
    z1.setflags(write=False)
    return z0, z1


def test_restated_normals_have_the_moments_of_a_standard_normal(normals):
    """each statistic within 5 standard errors of its exact value: mean 0 (se 1 / sqrt N), variance 1 (se sqrt(2 / N)),
    excess kurtosis 0 (se sqrt(24 / N)); the draws are bounded by the smallest u1 = 2^-24"""
    z, _ = normals
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    print(f"mean {mean:.3e} (se {1 / math.sqrt(N):.1e}), var - 1 {var - 1:.3e} (se {math.sqrt(2 / N):.1e}), "
          f"excess kurtosis {kurt:.3e} (se {math.sqrt(24 / N):.1e}), max |z| {np.abs(z).max():.4f}")
    assert abs(mean) <= 5.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    assert abs(kurt) <= 5.0 * math.sqrt(24.0 / N)
    assert np.abs(z).max() <= math.sqrt(48.0 * math.log(2.0)) * (1.0 + 1e-12)      # (fp64 rounding of the bound itself)


def test_restated_normals_are_uncorrelated_along_the_group_index_and_along_the_offset(normals):
    """lag-1 correlation 0 within 5 standard errors (1 / sqrt(pairs)): neighbouring elements, the same lane of neighbouring
    groups (counter word g -> g + 1), and the same element one offset later (counter word offset -> offset + 1)"""
    z, z_next = normals

    def corr(a, b):
        return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))

    for name, a, b in (("element", z[:-1], z[1:]), ("group", z[:-4], z[4:]), ("offset", z, z_next)):
        c = corr(a, b)
        print(f"lag-1 correlation along the {name}: {c:.3e} (se {1 / math.sqrt(a.size):.1e})")
        assert abs(c) <= 5.0 / math.sqrt(a.size)


def test_partial_tail_group_uses_its_leading_outputs_and_levels_use_consecutive_offsets():
    full = R.normals(9, 2, 8)
    assert np.array_equal(R.normals(9, 2, 6), full[:6])
    assert np.array_equal(R.normals(9, 2, 4, first_group=1), full[4:])
    xi = R.draw(9, (1 << 64) - 1, 2, 2, (3,))                     # the offset wraps modulo 2^64
    assert np.array_equal(xi[:, 0].ravel(), R.normals(9, (1 << 64) - 1, 6)) and np.array_equal(xi[:, 1].ravel(), R.normals(9, 0, 6))


def test_restated_replace_recurrence_equals_the_toeplitz_discount_product():
    rng = np.random.default_rng(0)
    B, T, C, L, M = 2, 4, 3, 5, 4
    xi = rng.standard_normal((B, T, C, L, M, 2))
    sigma, phi = rng.random((C, L)) + 0.5, np.array([0.2, 0.6, 0.9])
    eta = sigma[None, None, :, :, None, None] * xi
    eta[:, 0] /= np.sqrt(1 - phi ** 2)[None, :, None, None, None]
    lag = np.arange(T)[:, None] - np.arange(T)[None, :]
    discount = np.where(lag >= 0, phi[:, None, None] ** np.maximum(lag, 0), 0.0)
    want = np.einsum("ctr,brclmu->btclmu", discount, eta)
    assert R.rel_l2(R.update(None, xi, "replace", sigma, phi), want) < 1e-14


# ---- the modules against the reference's fixtures -------------------------------------------------------------------------
GOLDEN, CASES, build_case = R.GOLDEN, R.CASES, R.build_case


def test_the_fixture_holds_the_cases_the_processes_are_checked_on():
    metas = [json.loads(str(GOLDEN[f"{c}/meta"])) for c in CASES]
    assert {m["cls"] for m in metas} == {"DiffusionNoiseS2", "IsotropicGaussianRandomFieldS2", "DummyNoiseS2"}
    assert any(m["kwargs"]["num_time_steps"] == 3 and m["updates"] == [True, False, False] for m in metas)
    assert any(isinstance(m["kwargs"].get("kT"), list) for m in metas) and any(m["kwargs"].get("reflect") for m in metas)
    assert any(m["kwargs"].get("learnable") for m in metas)


@pytest.mark.parametrize("case", CASES)
def test_buffers_equal_the_references(case):
    """sigma_l, phi, discount: the reference's values within fp32 rounding (rtol 1e-6), shapes, dtypes, non-persistent
    buffers (parameters with the reference's annotation when learnable); the state starts as the reference's zeros"""
    m, meta = build_case(case)
    for name in ("sigma_l", "phi", "discount"):
        key = f"{case}/{name}"
        if key not in GOLDEN.files:
            assert not hasattr(m, name), f"{name} exists here but not in the reference"
            continue
        want = GOLDEN[key]
        got = getattr(m, name)
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32 and want.dtype == np.float32
        np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-6, atol=0.0)
        assert name not in m.state_dict() or isinstance(got, torch.nn.Parameter)
        if meta["kwargs"].get("learnable", False):
            assert meta["cls"] == "IsotropicGaussianRandomFieldS2", "the learnable fixture is the isotropic field's"
            assert isinstance(got, torch.nn.Parameter) and got.sharded_dims_mp == [None, None, None, "h", "w"]
        else:
            assert name in m._non_persistent_buffers_set
    init = GOLDEN[f"{case}/state_init"]
    assert tuple(m.state.shape) == init.shape and m.state.dtype == torch.float32 and not m.state.any()
    assert "state" in m._non_persistent_buffers_set and "rng" in m._non_persistent_buffers_set
    assert tuple(m.get_tensor_state().shape) == init.shape
    assert m.is_stateful() == (meta["cls"] == "DiffusionNoiseS2")


def test_attributes_and_repr_follow_the_reference():
    import makani_amd as ma
    m = ma.DiffusionNoiseS2((9, 16), 2, 3, num_time_steps=2, lmax=6, grid_type="legendre-gauss", reflect=True)
    assert (m.lmax, m.mmax, m.lmax_local, m.mmax_local, m.nlat_local, m.nlon_local) == (6, 6, 6, 6, 9, 16)
    assert (m.num_channels, m.num_time_steps, m.reflect, m.sigma, m.lambd, m.learnable) == (3, 2, True, 1.0, 1.0, False)
    assert m.kT == 0.5 * (500.0 / 6370.0) ** 2
    assert m.extra_repr() == (f"img_shape=(9, 16), num_channels=3, num_time_steps=2, lmax=6, reflect=True, sigma=1.0, "
                              f"kT={m.kT}, lambd=1.0, learnable=False")
    w = ma.IsotropicGaussianRandomFieldS2((9, 16), 1, 2)
    assert (w.sigma, w.alpha, w.learnable, w.num_time_steps, w.lmax, w.mmax) == (1.0, 0.0, False, 1, 9, 9)
    assert w.extra_repr().endswith("sigma=1.0, alpha=0.0, learnable=False")
    d = ma.DummyNoiseS2((9, 16), 2, 3, num_time_steps=2)
    assert d.mode == "constant_zero" and tuple(d.state.shape) == (2, 2, 3, 9, 16) and d.extra_repr().endswith("mode=constant_zero")
    with pytest.raises(NotImplementedError):
        ma.BaseNoiseS2((9, 16), 1, 1, 1).is_stateful()


def test_learnable_diffusion_parameters_carry_the_references_annotations():
    import makani_amd as ma
    fixed = ma.DiffusionNoiseS2((9, 16), 2, 2, kT=[0.01, 0.02])
    m = ma.DiffusionNoiseS2((9, 16), 2, 2, kT=[0.01, 0.02], learnable=True)
    assert isinstance(m.phi, torch.nn.Parameter) and isinstance(m.sigma_l, torch.nn.Parameter)
    assert m.phi.is_shared_mp == ["matmul", "h", "w"] and m.phi.sharded_dims_mp == [None, None, None]
    assert m.sigma_l.is_shared_mp == ["matmul", "w"] and m.sigma_l.sharded_dims_mp == [None, None, None, "h", None, None]
    assert torch.equal(m.phi.detach(), fixed.phi) and torch.equal(m.sigma_l.detach(), fixed.sigma_l)
    assert tuple(m.phi.shape) == (2, 1, 1, 1) and tuple(m.sigma_l.shape) == (1, 1, 2, 9, 1, 1)
    with pytest.raises(NotImplementedError, match="num_time_steps>1"):
        ma.DiffusionNoiseS2((9, 16), 2, 2, num_time_steps=2, learnable=True)


def test_error_cases():
    import makani_amd as ma
    for arg in ("kT", "lambd"):
        with pytest.raises(ValueError, match=f"expected {arg} to have 3 entries"):
            ma.DiffusionNoiseS2((9, 16), 2, 3, **{arg: [0.1, 0.2]})
        with pytest.raises(ValueError, match=f"expected {arg} to be a 1D tensor"):
            ma.DiffusionNoiseS2((9, 16), 2, 2, **{arg: [[0.1, 0.2]]})
    with pytest.raises(ValueError, match="unknown mode 'noisy'"):
        ma.DummyNoiseS2((9, 16), 2, 3, mode="noisy")
    m = ma.DiffusionNoiseS2((9, 16), 2, 3)
    with pytest.raises(ValueError, match="shape mismatch beyond batch dim"):
        m.set_tensor_state(torch.zeros(2, 1, 3, 9, 8, 2))
    assert tuple(m.state.shape) == (2, 1, 3, 9, 9, 2)                        # untouched by the refused call
    for mod in (m, ma.IsotropicGaussianRandomFieldS2((9, 16), 2, 3), ma.DummyNoiseS2((9, 16), 2, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod.update()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod()


def test_tensor_state_round_trip_resizes_the_batch_and_reset_zeroes():
    import makani_amd as ma
    m = ma.DiffusionNoiseS2((9, 16), 2, 3)
    new = torch.randn(5, 1, 3, 9, 9, 2)
    m.set_tensor_state(new)
    got = m.get_tensor_state()
    assert torch.equal(got, new) and got.data_ptr() != m.state.data_ptr() and "state" in m._non_persistent_buffers_set
    m.reset()
    assert tuple(m.state.shape) == (5, 1, 3, 9, 9, 2) and not m.state.any()
    m.reset(batch_size=3)
    assert tuple(m.state.shape) == (3, 1, 3, 9, 9, 2)
    before = m.state
    m._ensure_state(3)
    assert m.state is before


def test_rng_state_is_a_seed_offset_pair_and_no_torch_generator():
    import makani_amd as ma
    from makani_amd.stepper import _private_generators
    m = ma.DiffusionNoiseS2((9, 16), 2, 3, seed=17)
    assert m.rng.dtype == torch.int64 and m.rng.tolist() == [17, 0] and "rng" not in m.state_dict()
    cpu_state, gpu_state = m.get_rng_state()
    assert cpu_state is None and gpu_state.tolist() == [17, 0] and gpu_state.data_ptr() != m.rng.data_ptr()
    m.set_rng_state(None, torch.tensor([5, (1 << 32) - 1]))
    assert m.rng.tolist() == [5, (1 << 32) - 1]
    m.set_rng_state(*(cpu_state, gpu_state))
    assert m.rng.tolist() == [17, 0]
    m.set_rng_state(None, None)
    assert m.rng.tolist() == [17, 0]
    m.set_rng(4)
    assert m.rng.tolist() == [4, 0]
    assert _private_generators(torch.nn.Sequential(m)) == []


def test_a_spatial_group_larger_than_one_is_refused(monkeypatch):
    import makani_amd as ma
    from makani_amd import comm
    monkeypatch.setitem(comm._GROUPS, "spatial", (None, 2, 0))
    with pytest.raises(NotImplementedError, match="serial only"):
        ma.DiffusionNoiseS2((9, 16), 2, 3)


def test_noise_seed_reflect_follows_the_rank_layout(monkeypatch):
    import makani_amd as ma
    from makani_amd import comm
    assert ma.noise_seed_reflect(False) == (333, False) and ma.noise_seed_reflect(True, seed_offset=10) == (343, True)
    for name, size, rank in (("model", 4, 3), ("data", 6, 5), ("ensemble", 2, 1), ("batch", 3, 2)):
        monkeypatch.setitem(comm._GROUPS, name, (None, size, rank))
    assert ma.noise_seed_reflect(False, seed_offset=1) == (333 + 1 + 3 + 4 * 5, False)
    assert ma.noise_seed_reflect(True) == (333 + 3 + 4 * 0 + 4 * 2 * 2, False)
    monkeypatch.setitem(comm._GROUPS, "ensemble", (None, 4, 2))
    assert ma.noise_seed_reflect(True) == (333 + 3 + 4 * 1 + 4 * 4 * 2, True)


def test_build_noise_dispatches_on_the_type():
    import makani_amd as ma
    kw = dict(img_shape=(9, 16), batch_size=2, num_channels=2, num_time_steps=2, grid_type="legendre-gauss", seed=9, reflect=True)
    d = ma.build_noise({"type": "diffusion", "kT": [0.1, 0.2], "lmax": 5}, default_lambd=0.25, **kw)
    assert isinstance(d, ma.DiffusionNoiseS2) and d.lambd == 0.25 and d.kT == [0.1, 0.2] and d.lmax == 5 and d.reflect
    assert d.rng.tolist() == [9, 0] and d.isht.grid == "legendre-gauss"
    assert ma.build_noise({"type": "diffusion"}, **kw).kT == 0.5 * (100 / 6370) ** 2
    w = ma.build_noise({"type": "white", "alpha": 2.0, "sigma": 3.0, "learnable": True}, **kw)
    assert isinstance(w, ma.IsotropicGaussianRandomFieldS2) and (w.alpha, w.sigma, w.learnable) == (2.0, 3.0, True)
    z = ma.build_noise({"type": "dummy"}, **kw)
    assert isinstance(z, ma.DummyNoiseS2) and z.mode == "constant_zero" and not z.reflect
    with pytest.raises(ValueError, match="specify a noise type"):
        ma.build_noise({}, **kw)
    with pytest.raises(NotImplementedError, match="pink"):
        ma.build_noise({"type": "pink"}, **kw)


def test_library_validates_noise_arguments_on_the_host():
    from makani_amd._lib import lib
    L, p, null = lib(), ctypes.c_void_p(64), ctypes.c_void_p(0)
    assert L.mk_noise_update(null, null, p, p, p, 1, 1, 1, 1, 4, 4, 0, None) < 0 and b"null state" in L.mk_last_error()
    assert L.mk_noise_update(p, null, p, p, null, 1, 1, 1, 1, 4, 4, 0, None) < 0 and b"null rng" in L.mk_last_error()
    assert L.mk_noise_update(p, null, null, p, p, 1, 1, 1, 1, 4, 4, 0, None) < 0 and b"null sigma" in L.mk_last_error()
    assert L.mk_noise_update(p, null, p, p, p, 1, 1, 0, 1, 4, 4, 0, None) < 0 and b"T >= 1" in L.mk_last_error()
    assert L.mk_noise_update(p, null, p, p, p, 3, 1, 1, 1, 4, 4, 0, None) < 0 and b"unknown mode 3" in L.mk_last_error()
    assert L.mk_noise_update(p, null, p, p, p, 0, 1, 1, 1 << 15, 1 << 8, 1 << 8, 0, None) < 0 and b"2^31" in L.mk_last_error()
    assert L.mk_noise_advance(null, 1, None) < 0 and b"null pointer" in L.mk_last_error()


# ---- InputNoise over a stub process ---------------------------------------------------------------------------------------
class StubNoise(torch.nn.Module):
    def __init__(self, B, T, C, H, W, stateful):
        super().__init__()
        self.register_buffer("state", torch.zeros(B, T, C, 2, 2, 2), persistent=False)
        self.dims, self.stateful, self.calls = (T, C, H, W), stateful, []

    def is_stateful(self):
        return self.stateful

    def update(self, replace_state=False, batch_size=None):
        self.calls.append((replace_state, batch_size))
        if batch_size is not None:
            self.state = torch.zeros(batch_size, *self.state.shape[1:])

    def forward(self):
        T, C, H, W = self.dims
        return torch.arange(self.state.shape[0] * T * C * H * W, dtype=torch.float32).reshape(self.state.shape[0], T, C, H, W) + 1.0


def test_input_noise_concatenates_per_time_level():
    import makani_amd as ma
    B, T, C, H, W = 2, 2, 3, 4, 6
    stub = StubNoise(B, T, 2, H, W, True)
    mod = ma.InputNoise(stub, mode="concatenate", n_history=T - 1)
    x, xc = torch.randn(B, T, C, H, W), torch.randn(B, T, 1, H, W)
    out = mod(x, xc)
    assert tuple(out.shape) == (B, T, C + 1 + 2, H, W)
    assert torch.equal(out[:, :, :C], x) and torch.equal(out[:, :, C:C + 1], xc) and torch.equal(out[:, :, C + 1:], stub())
    assert torch.equal(mod(x), torch.cat([x, stub()], dim=2))
    flat = mod(x.flatten(1, 2), xc.flatten(1, 2))                          # 4-d input: the history stays folded into the channels
    assert tuple(flat.shape) == (B, T * (C + 3), H, W) and torch.equal(flat, out.flatten(1, 2))


def test_input_noise_perturbs_out_of_place():
    import makani_amd as ma
    B, T, C, H, W = 2, 1, 4, 3, 4
    stub = StubNoise(B, T, 2, H, W, False)
    mod = ma.InputNoise(stub, mode="perturb", perturb_channels=[3, 1])
    x = torch.randn(B, T, C, H, W)
    keep = x.clone()
    out = mod(x)
    assert torch.equal(x, keep) and tuple(out.shape) == x.shape
    n = stub()
    assert torch.equal(out[:, :, 3], x[:, :, 3] + n[:, :, 0]) and torch.equal(out[:, :, 1], x[:, :, 1] + n[:, :, 1])
    assert torch.equal(out[:, :, [0, 2]], x[:, :, [0, 2]])


def test_input_noise_error_logic():
    import makani_amd as ma
    stub = StubNoise(2, 1, 2, 3, 4, True)
    mod = ma.InputNoise(stub)
    with pytest.raises(RuntimeError, match=r"batch mismatch between input_noise state \(2\) and input \(3\)"):
        mod(torch.zeros(3, 1, 5, 3, 4))
    with pytest.raises(RuntimeError, match="refusing to resize"):
        mod.update_internal_state(batch_size=3)
    assert stub.calls == []
    mod.update_internal_state(batch_size=2)                       # same size: nothing to refuse
    mod.update_internal_state(replace_state=True, batch_size=3)
    mod.update_internal_state()
    assert stub.calls == [(False, 2), (True, 3), (False, None)] and stub.state.shape[0] == 3
    stateless = StubNoise(2, 1, 2, 3, 4, False)
    ma.InputNoise(stateless).update_internal_state(batch_size=5)  # white / dummy noise redraws anyway
    assert stateless.calls == [(False, 5)]
    with pytest.raises(NotImplementedError, match="mode replace"):
        ma.InputNoise(stub, mode="replace")
    with pytest.raises(ValueError, match="perturb"):
        ma.InputNoise(stub, mode="perturb")
