"""The input noise inside the rollout wrappers (makani_amd/stepper.py with makani_amd.noise.InputNoise) on the GPU, one process:
9 x 16 grid, a two-layer 1x1-convolution network, DiffusionNoiseS2 with a history of two levels.  The wrapper's rollout against a
hand-written unroll driven by a second noise module of the same seed, bit for bit (the update order of
makani/models/stepper.py:226-315), and rollout checkpointing against the plain rollout."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMG, B, C, NH, NF, NOISE_C = (9, 16), 2, 3, 1, 2, 2
T = NH + 1
PERTURB = [2, 0]


class _Conv1x1(torch.nn.Linear):
    """a 1x1 convolution as the matrix product over the channel axis it is"""

    def forward(self, x):
        return super().forward(x.movedim(1, -1)).movedim(-1, 1)


def _net(cin):
    torch.manual_seed(4)
    return torch.nn.Sequential(_Conv1x1(cin, 8), torch.nn.Tanh(), _Conv1x1(8, C)).to(DEV)


def _process(seed=5):
    import makani_amd as ma
    return ma.DiffusionNoiseS2(IMG, B, NOISE_C, num_time_steps=T, kT=[1e-3, 4e-3], lambd=[0.5, 1.0], seed=seed).to(DEV)


def _stage(mode, seed=5):
    import makani_amd as ma
    return ma.InputNoise(_process(seed), mode=mode, perturb_channels=PERTURB if mode == "perturb" else None, n_history=NH)


def _noised(window, n, mode):
    """what the network sees: the window (B, T C, H, W) with the field n (B, T, NOISE_C, H, W) appended / added per time level"""
    x = window.reshape(window.shape[0], T, C, *IMG)
    if mode == "concatenate":
        return torch.cat([x, n], dim=2).flatten(1, 2)
    x = x.clone()
    x[:, :, PERTURB] += n
    return x.flatten(1, 2)


def _unroll(net, twin, x, mode, update_state=True, replace_state=True):
    if update_state:
        twin.update(replace_state=replace_state)
    window, preds = x, []
    for step in range(NF + 1):
        preds.append(net(_noised(window, twin(), mode)))
        if step < NF:
            twin.update()
            window = torch.cat([window[:, C:], preds[-1]], dim=1)
    return torch.cat(preds, dim=1)


@pytest.mark.parametrize("mode", ["concatenate", "perturb"])
def test_rollout_with_input_noise_equals_a_hand_written_unroll(mode):
    from makani_amd.stepper import MultiStepWrapper, SingleStepWrapper
    net = _net(T * (C + NOISE_C) if mode == "concatenate" else T * C)
    stage, twin = _stage(mode), _process()
    wrap = MultiStepWrapper(net, n_future=NF, n_history=NH, input_noise=stage).train()
    x = torch.randn(B, T * C, *IMG, device=DEV)
    keep = x.clone()
    with torch.no_grad():
        y = wrap(x)
        assert tuple(y.shape) == (B, (NF + 1) * C, *IMG) and torch.equal(x, keep)
        assert torch.equal(y, _unroll(net, twin, x, mode))
        assert stage.input_noise.rng.tolist() == twin.rng.tolist() == [5, T + NF]
        # the next sample continues the process (one autoregressive step first), or leaves it where it is
        assert torch.equal(wrap(x, replace_state=False), _unroll(net, twin, x, mode, replace_state=False))
        assert torch.equal(wrap(x, update_state=False), _unroll(net, twin, x, mode, update_state=False))
        assert torch.equal(stage.input_noise.state, twin.state) and twin.rng.tolist() == [5, T + 3 * NF + 1]
        assert not torch.equal(wrap(x), y)                    # a fresh state from a later offset
        twin.update(replace_state=True)
        for _ in range(NF):
            twin.update()

        # evaluation: one step, the state sized to the call's batch
        wrap.eval()
        x5 = torch.randn(5, T * C, *IMG, device=DEV)
        y5 = wrap(x5)
        twin.update(replace_state=True, batch_size=5)
        assert stage.input_noise.state.shape[0] == 5 and torch.equal(stage.input_noise.state, twin.state)
        assert tuple(y5.shape) == (5, C, *IMG) and torch.equal(y5, net(_noised(x5, twin(), mode)))
        assert torch.equal(wrap(x5, update_state=False), y5)
        with pytest.raises(RuntimeError, match="refusing to resize"):
            wrap(x, replace_state=False)

        single = SingleStepWrapper(net, input_noise=stage)
        ys = single(x)
        twin.update(replace_state=True, batch_size=B)
        assert torch.equal(ys, net(_noised(x, twin(), mode))) and torch.equal(single(x, update_state=False), ys)


def test_rollout_checkpointing_with_input_noise_is_exact_and_draws_nothing_in_the_recompute():
    from makani_amd.stepper import MultiStepWrapper
    net = _net(T * (C + NOISE_C))
    x = torch.randn(B, T * C, *IMG, device=DEV)
    g = torch.randn(B, (NF + 1) * C, *IMG, device=DEV)
    grads, outs, counters = [], [], []
    for checkpointed in (False, True):
        stage = _stage("concatenate")
        wrap = MultiStepWrapper(net, n_future=NF, n_history=NH, multistep_checkpoint=checkpointed, input_noise=stage).train()
        net.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_(True)
        y = wrap(xs)
        counters.append(stage.input_noise.rng.tolist())
        (y * g).sum().backward()
        counters.append(stage.input_noise.rng.tolist())       # the recompute of the backward pass drew nothing
        outs.append(y.detach())
        grads.append([p.grad.clone() for p in net.parameters()] + [xs.grad.clone()])
    assert torch.equal(outs[0], outs[1])
    assert all(torch.equal(a, b) and bool(a.any()) for a, b in zip(*grads))
    assert counters == [[5, T + NF]] * 4
