"""GPU tests of the input-noise processes (makani_amd/noise.py over csrc/noise.hip): parity with the reference's own classes
driven by their recorded innovations (tests/golden/noise.npz, tools/make_noise_golden.py), the generator against the fp64
restatement of tests/_noise_ref.py from the same (seed, offset), the counter's carry, bitwise properties and replay from a
captured graph.  Gate: the project's fp32 operator tolerance, rel-L2 <= 1e-5,
with torch's tf32 switch cleared."""
import pytest
import torch

import _noise_ref as R
from _noise_ref import CASES, GOLDEN, build_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


@pytest.fixture(autouse=True)
def _three_limbs():
    was = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = was


def _err(got, want, what):
    err = R.rel_l2(got.detach().cpu().numpy(), want)
    print(f"{what}: rel-L2 {err:.2e}")
    return err


# ---- parity with the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_updates_and_field_match_the_reference_on_its_own_innovations(case):
    m, meta = build_case(case)
    m = m.to(DEV)
    for k, replace in enumerate(meta["updates"]):
        counter = m.rng.clone()
        m.update(replace_state=replace, innovation=torch.from_numpy(GOLDEN[f"{case}/xi_{k}"]))
        assert _err(m.state, GOLDEN[f"{case}/state_{k}"], f"{case} state after update {k}") <= TOL
        assert torch.equal(m.rng, counter), "given innovations must not advance the counter"
    field = m()
    assert tuple(field.shape) == GOLDEN[f"{case}/field"].shape and field.dtype == torch.float32
    assert _err(field, GOLDEN[f"{case}/field"], f"{case} field") <= TOL
    if f"{case}/sigma_l_grad" in GOLDEN.files:
        g = torch.from_numpy(GOLDEN[f"{case}/g"]).to(DEV)
        (grad,) = torch.autograd.grad((field * g).sum(), m.sigma_l)
        assert _err(grad, GOLDEN[f"{case}/sigma_l_grad"], f"{case} sigma_l gradient") <= TOL


# ---- the generator against the restatement --------------------------------------------------------------------------------
def _diffusion(B, T, C, L, seed=333, **kw):
    """L = M = lmax on the smallest grid of the fixtures that carries it; distinct, slowly decaying spectra per channel"""
    import makani_amd as ma
    img = (9, 16) if L <= 9 else (33, 64)
    m = ma.DiffusionNoiseS2(img, B, C, num_time_steps=T, lmax=L, kT=[1e-3 * (c + 1) for c in range(C)],
                            lambd=[0.5 + 0.5 * c for c in range(C)], seed=seed, **kw).to(DEV)
    assert (m.lmax, m.mmax) == (L, L)
    return m


def _tables(m):
    return (m.sigma_l.detach().double().cpu().numpy().reshape(m.num_channels, m.lmax),
            m.phi.detach().double().cpu().numpy().reshape(-1))


@pytest.mark.parametrize("B, T, C, L", [
    (1, 1, 3, 5),       # 150 floats: a tail group, a channel stride that is no multiple of 4, the scalar path
    (2, 2, 3, 5),       # the scalar path with groups that straddle batch entries, and a history
    (2, 3, 2, 33),      # several blocks, groups that straddle degree and channel boundaries, T > 1
    (2, 1, 2, 8),       # the vector path, everything aligned
])
def test_drawn_states_match_the_restatement_from_the_same_seed_and_offset(B, T, C, L):
    seed, offset = 2025, 40
    m = _diffusion(B, T, C, L, seed=seed)
    m.set_rng_state(None, torch.tensor([seed, offset]))
    sigma, phi = _tables(m)
    inner = (C, L, L, 2)
    m.update(replace_state=True)
    want = R.update(None, R.draw(seed, offset, T, B, inner), "replace", sigma, phi)
    assert _err(m.state, want, "replace") <= TOL
    m.update()
    want = R.update(want, R.draw(seed, offset + T, 1, B, inner), "ar", sigma, phi)
    assert _err(m.state, want, "autoregressive step") <= TOL
    assert m.get_rng_state()[1].tolist() == [seed, offset + T + 1]


def test_white_and_dummy_draws_match_the_restatement():
    import makani_amd as ma
    w = ma.IsotropicGaussianRandomFieldS2((9, 16), 2, 3, num_time_steps=2, seed=12, reflect=True).to(DEV)
    w.update()
    assert _err(w.state, R.update(None, R.draw(12, 0, 2, 2, (3, 9, 9, 2)), "white", reflect=True), "white") <= TOL
    assert w.rng.tolist() == [12, 2]
    d = ma.DummyNoiseS2((9, 16), 2, 3, num_time_steps=2, mode="constant_random", seed=13).to(DEV)
    d.update()
    assert _err(d.state, R.draw(13, 0, 2, 2, (3, 9, 16)), "dummy constant_random") <= TOL
    assert d() is d.state
    z = ma.DummyNoiseS2((9, 16), 2, 3).to(DEV)
    z.state.fill_(1.0)
    z.update()
    assert not z().any()


def test_counter_carries_into_the_high_word():
    seed, offset = (5 << 32) + 7, (1 << 32) - 1
    m = _diffusion(2, 1, 2, 8, seed=seed)
    m.set_rng_state(None, torch.tensor([seed, offset]))
    sigma, phi = _tables(m)
    m.update(replace_state=True)
    want = R.update(None, R.draw(seed, offset, 1, 2, (2, 8, 8, 2)), "replace", sigma, phi)
    assert _err(m.state, want, "offset 2^32 - 1") <= TOL
    m.update()
    want = R.update(want, R.draw(seed, offset + 1, 1, 2, (2, 8, 8, 2)), "ar", sigma, phi)
    assert _err(m.state, want, "offset 2^32") <= TOL
    cpu_state, gpu_state = m.get_rng_state()
    assert cpu_state is None and gpu_state.tolist() == [seed, (1 << 32) + 1]


# ---- bitwise properties ---------------------------------------------------------------------------------------------------
def _run(m, steps=2):
    m.update(replace_state=True)
    for _ in range(steps):
        m.update()
    return m.get_tensor_state()


def test_seed_decides_the_stream_and_reflect_negates_it_exactly():
    a, b = _run(_diffusion(2, 3, 2, 33, seed=1)), _run(_diffusion(2, 3, 2, 33, seed=1))
    assert torch.equal(a, b) and bool(a.abs().sum() > 0)
    assert not torch.equal(a, _run(_diffusion(2, 3, 2, 33, seed=2)))
    assert torch.equal(_run(_diffusion(2, 3, 2, 33, seed=1, reflect=True)), -a)
    assert torch.equal(_run(_diffusion(2, 1, 2, 8, seed=1, learnable=True)), _run(_diffusion(2, 1, 2, 8, seed=1)))


def test_saved_rng_and_tensor_state_continue_bit_identically():
    m = _diffusion(2, 2, 3, 5)
    m.update(replace_state=True)
    rng_state, tensor_state = m.get_rng_state(), m.get_tensor_state()
    first = _run_steps(m)
    m.set_rng_state(*rng_state)
    m.set_tensor_state(tensor_state)
    assert torch.equal(_run_steps(m), first)
    other = _diffusion(3, 2, 3, 5, seed=99)                      # another module, another batch size: state and counter move over
    other.set_rng_state(*rng_state)
    other.set_tensor_state(tensor_state)
    assert torch.equal(_run_steps(other), first)


def _run_steps(m):
    m.update()
    m.update()
    return m.get_tensor_state()


def test_reset_zeroes_the_state_and_resizes_the_batch():
    m = _diffusion(2, 1, 2, 8)
    m.update(replace_state=True)
    assert bool(m.state.any())
    m.reset()
    assert tuple(m.state.shape) == (2, 1, 2, 8, 8, 2) and not m.state.any()
    m.reset(batch_size=5)
    assert tuple(m.state.shape) == (5, 1, 2, 8, 8, 2) and m.state.is_cuda and not m.state.any()
    m.update(replace_state=True, batch_size=3)
    assert tuple(m.state.shape) == (3, 1, 2, 8, 8, 2) and bool(m.state.any())
    assert tuple(m().shape) == (3, 1, 2, 9, 16)


def test_forward_returns_the_field_of_the_old_state_and_then_advances():
    m, twin = _diffusion(2, 2, 2, 8), _diffusion(2, 2, 2, 8)
    m.update(replace_state=True)
    twin.update(replace_state=True)
    old = m()
    assert torch.equal(m(update_internal_state=True), old)
    twin.update()
    assert torch.equal(m.state, twin.state) and m.rng.tolist() == [333, 3]
    assert torch.equal(m(), twin()) and not torch.equal(m(), old)


# ---- hipGraph -------------------------------------------------------------------------------------------------------------
def test_update_and_forward_replay_from_a_captured_graph_with_fresh_draws():
    m, eager = _diffusion(2, 2, 2, 33), _diffusion(2, 2, 2, 33)
    for mod in (m, eager):                                       # also loads every kernel of the sequence outside the capture
        mod.update(replace_state=True)
        mod.update()
        mod()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            m.update()
            out = m()
    torch.cuda.current_stream().wait_stream(stream)
    assert torch.equal(m.state, eager.state), "capturing must not run the update"
    states = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        eager.update()
        want = eager()
        assert torch.equal(m.state, eager.state) and torch.equal(out, want)
        states.append(m.get_tensor_state())
    assert not torch.equal(states[0], states[1]) and not torch.equal(states[1], states[2]) and not torch.equal(states[0], states[2])
    assert m.rng.tolist() == eager.rng.tolist() == [333, 6]
