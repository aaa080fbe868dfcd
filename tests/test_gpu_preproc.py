"""``Preprocessor2D`` and the kernels of csrc/preproc.hip on the GPU against the fp64 restatement tests/_preproc_ref.py.

Grids: 13 x 22 (HW = 286 = 2 mod 4: every second plane starts off a 16-byte boundary, scalar path, fewer pixels than one chunk),
33 x 64 (two chunks of the streaming kernels, 16-byte path) and 91 x 180 (eight chunks, the last one short; two chunks of 8192
pixels in the reduction kernels, merged by Chan's formula).  B = 2, C = 3.

Gates (relative L2): statistics 1e-6 against fp64; the assembled input 1e-6 against the fp64 normalisation evaluated with the
kernel's own fp32 mu / sigma, and 4 * 2^-24 * (1 + max |mu| / sigma) against the all-fp64 result (what one fp32 rounding of mu
costs); bf16 output 2^-8; finish and every gradient 1e-5 (the project's gate for an fp32 operation)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _preproc_ref as ref          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C = 2, 3
GRIDS = [(13, 22), (33, 64), (91, 180)]
F64 = torch.float64


class _ParamNoise(torch.nn.Module):
    """a noise process whose field is a parameter: known values, and a leaf for the gradient of learnable noise"""

    def __init__(self, shape, dtype=torch.float32, seed=7):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.state = torch.nn.Parameter((0.7 * torch.randn(shape, generator=g) + 0.3).to(dtype))

    def forward(self):
        return self.state

    def update(self, replace_state=False, batch_size=None):
        pass

    def is_stateful(self):
        return False


def _field(shape, ratio, gen, chan_dim):
    """seeded values with per-channel sigma in [0.5, 2] and mean = +-ratio sigma (|mu| / sigma <= ratio, no constant channel)"""
    nch = shape[chan_dim]
    view = [1] * len(shape)
    view[chan_dim] = nch
    sigma = (0.5 + 1.5 * torch.rand(nch, generator=gen)).reshape(view)
    sign = (torch.arange(nch) % 2 * 2 - 1).reshape(view)
    return torch.randn(shape, generator=gen) * sigma + ratio * sign * sigma


def _case(grid, mode, nh, U, N, S, ratio=3.0, dtype=torch.float32, bias=True, seed=0):
    """module on the GPU, its inputs, and the same values in fp64 for the restatement"""
    import makani_amd as ma
    H, W = grid
    T = nh + 1
    gen = torch.Generator().manual_seed(1000 * H + 100 * nh + 10 * U + N + S + seed)
    win = _field((B, T, C, H, W), ratio, gen, 2).flatten(1, 2).to(dtype)
    unp = _field((B, T, U, H, W), ratio, gen, 2).to(dtype) if U else None
    tar = _field((B, 2, U, H, W), ratio, gen, 2).to(dtype) if U else None
    static = torch.randn((1, S, H, W), generator=gen) if S else None
    bias_t = 0.2 * torch.randn((1, C, H, W), generator=gen) if bias else None
    noise = ma.InputNoise(_ParamNoise((B, T, N, H, W), dtype), mode="concatenate", n_history=nh) if N else None
    pre = ma.Preprocessor2D(img_shape=grid, n_history=nh, history_normalization_mode=mode,
                            history_normalization_decay=0.5 if mode == "exponential" else None, static_features=static,
                            bias_correction=bias_t, input_noise=noise).to(DEV)
    pre.train()
    if U:
        pre.cache_unpredicted_features(None, None, unp.to(DEV), tar.to(DEV))
    r = dict(win=win.double(), unp=None if unp is None else unp.double(), tar=None if tar is None else tar.double(),
             noi=None if noise is None else noise.input_noise.state.detach().double().cpu(),
             static=None if static is None else static[0].double(), bias=None if bias_t is None else bias_t[0].double(),
             q=ref.quad_weights(H, W), wt=None if mode == "none" else ref.time_weights(mode, nh, 0.5), T=T)
    return pre, win.to(DEV), r


def _ref_assemble(r, mode, **kw):
    return ref.assemble(r["win"], r["unp"], r["noi"], r["static"], r["T"], mode, r["q"], r["wt"], **kw)


@pytest.mark.parametrize("nh", [0, 2])
@pytest.mark.parametrize("mode", ["none", "mean", "exponential"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_assemble_statistics_and_finish_against_fp64(grid, mode, nh):
    for U in (0, 2):
        for N in (0, 1):
            for S in (0, 5):
                pre, win, r = _case(grid, mode, nh, U, N, S)
                J = C + U + N
                with torch.no_grad():
                    out = pre.assemble(win)
                    gen = torch.Generator().manual_seed(5)
                    yn = torch.randn((B, C, *grid), generator=gen)
                    y = pre.finish(yn.to(DEV))
                want, mu, sigma = _ref_assemble(r, mode)
                assert tuple(out.shape) == (B, (nh + 1) * J + S, *grid) and out.dtype == torch.float32
                tag = f"{grid} {mode} nh={nh} U={U} N={N} S={S}"
                if mode == "none":
                    assert torch.equal(out.cpu().double(), want), tag          # a copy
                    assert tuple(pre.history_mean.shape) == (1, 1, 1, 1)
                    e_fin = ref.rel(y, ref.finish(yn.double(), r["bias"], None, None))
                    print(f"{tag}: finish {e_fin:.1e}")
                    assert e_fin <= 1e-5, tag
                    continue
                assert tuple(pre.history_mean.shape) == tuple(pre.history_std.shape) == (B, J, 1, 1)
                assert pre.history_mean.dtype == pre.history_std.dtype == torch.float32
                kmu, ksig = pre.history_mean.reshape(B, J).double().cpu(), pre.history_std.reshape(B, J).double().cpu()
                e_mu, e_sig = ref.rel(kmu, mu), ref.rel(ksig, sigma)
                own, _, _ = _ref_assemble(r, mode, mu=kmu, sigma=ksig)
                e_own, e_all = ref.rel(out, own), ref.rel(out, want)
                bound = 4 * 2.0 ** -24 * (1 + (mu.abs() / sigma).max().item())
                e_fin = ref.rel(y, ref.finish(yn.double(), r["bias"], kmu, ksig))
                print(f"{tag}: mean {e_mu:.1e} std {e_sig:.1e} out/own stats {e_own:.1e} out/fp64 {e_all:.1e} (bound {bound:.1e}) "
                      f"finish {e_fin:.1e}")
                assert e_mu <= 1e-6 and e_sig <= 1e-6, tag
                assert e_own <= 1e-6 and e_all <= bound, tag
                assert e_fin <= 1e-5, tag


@pytest.mark.parametrize("nh", [0, 2])
@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_statistics_of_a_field_a_thousand_sigma_off_zero(grid, nh):
    """|mu| / sigma = 1e3: a one-pass sum of squares minus the squared mean misses the std gate by orders of magnitude"""
    pre, win, r = _case(grid, "mean", nh, 2, 1, 0, ratio=1e3)
    with torch.no_grad():
        out = pre.assemble(win)
    want, mu, sigma = _ref_assemble(r, "mean")
    J = C + 3
    kmu, ksig = pre.history_mean.reshape(B, J).double().cpu(), pre.history_std.reshape(B, J).double().cpu()
    e_mu, e_sig = ref.rel(kmu, mu), ref.rel(ksig, sigma)
    own, _, _ = _ref_assemble(r, "mean", mu=kmu, sigma=ksig)
    ratio = (mu.abs() / sigma).max().item()
    bound = 4 * 2.0 ** -24 * (1 + ratio)
    e_own, e_all = ref.rel(out, own), ref.rel(out, want)
    print(f"{grid} nh={nh} ratio {ratio:.0f}: mean {e_mu:.1e} std {e_sig:.1e} out/own stats {e_own:.1e} out/fp64 {e_all:.1e} "
          f"(bound {bound:.1e})")
    assert ratio >= 900
    assert e_mu <= 1e-6 and e_sig <= 1e-6
    assert e_own <= 1e-6 and e_all <= bound


def test_bf16_sources_give_bf16_output_and_fp32_statistics():
    grid, mode, nh = (33, 64), "exponential", 2
    pre, win, r = _case(grid, mode, nh, 2, 1, 5, dtype=torch.bfloat16)
    with torch.no_grad():
        out = pre.assemble(win)
    want, mu, sigma = _ref_assemble(r, mode)
    J = C + 3
    assert out.dtype == torch.bfloat16 and pre.history_mean.dtype == torch.float32
    e_mu, e_sig = ref.rel(pre.history_mean.reshape(B, J), mu), ref.rel(pre.history_std.reshape(B, J), sigma)
    e_out = ref.rel(out, want)
    print(f"bf16: mean {e_mu:.1e} std {e_sig:.1e} out {e_out:.1e}")
    assert e_mu <= 1e-6 and e_sig <= 1e-6 and e_out <= 2.0 ** -8
    # the scalar path of the 2-byte loads: planes that start off an 8-byte boundary
    pre, win, r = _case((13, 22), "mean", 0, 2, 1, 5, dtype=torch.bfloat16)
    with torch.no_grad():
        out = pre.assemble(win)
    e_out = ref.rel(out, _ref_assemble(r, "mean")[0])
    print(f"bf16 13x22: out {e_out:.1e}")
    assert e_out <= 2.0 ** -8


def _losses(pre, win, grid, with_finish, seed=3):
    """sum(out r1) (+ sum(y r2) with y = finish(yn)): the value parts and the gradients w.r.t. window, noise and yn"""
    gen = torch.Generator().manual_seed(seed)
    win = win.clone().requires_grad_(True)
    out = pre.assemble(win)
    r1 = torch.randn(out.shape, generator=gen)
    yn = torch.randn((B, C, *grid), generator=gen)
    r2 = torch.randn((B, C, *grid), generator=gen)
    loss = (out * r1.to(DEV)).sum()
    leaves = [win] + ([pre.noise_stage.input_noise.state] if pre.noise_stage is not None else [])
    ynd = yn.to(DEV).requires_grad_(True)
    y = None
    if with_finish:
        y = pre.finish(ynd)
        loss = loss + (y * r2.to(DEV)).sum()
        leaves.append(ynd)
    grads = torch.autograd.grad(loss, leaves)
    return out, y, grads, (r1.double(), yn.double(), r2.double())


def _ref_losses(r, mode, rnd, with_finish):
    r1, yn, r2 = rnd
    win = r["win"].clone().requires_grad_(True)
    noi = None if r["noi"] is None else r["noi"].clone().requires_grad_(True)
    out, mu, sigma = ref.assemble(win, r["unp"], noi, r["static"], r["T"], mode, r["q"], r["wt"])
    loss = (out * r1).sum()
    leaves = [win] + ([noi] if noi is not None else [])
    yn = yn.clone().requires_grad_(True)
    y = None
    if with_finish:
        y = ref.finish(yn, r["bias"], mu, sigma)
        loss = loss + (y * r2).sum()
        leaves.append(yn)
    return out, y, torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("with_finish", [False, True], ids=["direct", "through-the-statistics"])
@pytest.mark.parametrize("nh", [0, 2])
@pytest.mark.parametrize("mode", ["none", "mean", "exponential"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_gradients_to_window_noise_and_prediction(grid, mode, nh, with_finish):
    """|mu| / sigma = 30; with ``with_finish`` the statistics also receive the gradient of the de-normalised prediction"""
    for U, N, S in ((2, 1, 5), (0, 0, 0), (0, 1, 0)):
        pre, win, r = _case(grid, mode, nh, U, N, S, ratio=30.0)
        out, y, grads, rnd = _losses(pre, win, grid, with_finish)
        wout, wy, wgrads = _ref_losses(r, mode, rnd, with_finish)
        names = ["window"] + (["noise"] if N else []) + (["yn"] if with_finish else [])
        errs = {n: ref.rel(g, w) for n, g, w in zip(names, grads, wgrads)}
        if with_finish:
            errs["finish"] = ref.rel(y, wy)
        print(f"{grid} {mode} nh={nh} U={U} N={N} S={S}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert len(grads) == len(wgrads) == len(names)
        assert all(g.shape == w.shape for g, w in zip(grads, wgrads))
        assert max(errs.values()) <= 1e-5, errs


@pytest.mark.parametrize("mode", ["none", "mean", "exponential"])
@pytest.mark.parametrize("grid", GRIDS[:2], ids=lambda g: f"{g[0]}x{g[1]}")
def test_assemble_equals_the_four_methods_and_repeats_bit_for_bit(grid, mode):
    pre, win, r = _case(grid, mode, 2, 2, 1, 5)
    out, y, grads, _ = _losses(pre, win, grid, True)
    mean, std = pre.history_mean.clone(), pre.history_std.clone()
    # the composition of the reference's wrapper (stepper.py:239-247, 261-267)
    w2 = win.clone().requires_grad_(True)
    inpa = pre.append_unpredicted_features(w2)
    pre.history_compute_stats(inpa)
    comp = pre.add_static_features(pre.history_normalize(inpa, target=False))
    assert torch.equal(comp, out) and torch.equal(pre.history_mean, mean) and torch.equal(pre.history_std, std)
    gen = torch.Generator().manual_seed(3)
    r1 = torch.randn(out.shape, generator=gen).to(DEV)
    yn = torch.randn((B, C, *grid), generator=gen).to(DEV).requires_grad_(True)
    r2 = torch.randn((B, C, *grid), generator=gen).to(DEV)
    ycomp = pre.history_denormalize(pre.correct_bias(yn), target=True)
    assert torch.equal(ycomp, y)
    leaves = [w2, pre.noise_stage.input_noise.state, yn]
    cgrads = torch.autograd.grad((comp * r1).sum() + (ycomp * r2).sum(), leaves)
    errs = [ref.rel(a, b) for a, b in zip(cgrads, grads)]
    print(f"{grid} {mode}: gradients of the composition against the fused path {errs}")
    assert max(errs) <= 1e-5          # (the composition adds its gradient parts in another order)
    # a second call of the fused path
    out2, y2, grads2, _ = _losses(pre, win, grid, True)
    assert torch.equal(out2, out) and torch.equal(y2, y) and all(torch.equal(a, b) for a, b in zip(grads2, grads))


def test_unpredicted_static_and_bias_tensors_that_require_grad_raise():
    pre, win, r = _case((13, 22), "mean", 0, 2, 0, 5)
    pre.unpredicted_inp_train.requires_grad_(True)
    with pytest.raises(RuntimeError, match="unpredicted features require grad"):
        pre.assemble(win)
    pre.unpredicted_inp_train.requires_grad_(False)
    pre.static_features.requires_grad_(True)
    with pytest.raises(RuntimeError, match="static_features requires grad"):
        pre.assemble(win)
    pre.static_features.requires_grad_(False)
    pre.assemble(win)
    pre.bias_correction.requires_grad_(True)
    with pytest.raises(RuntimeError, match="bias_correction requires grad"):
        pre.finish(torch.zeros((B, C, 13, 22), device=DEV))


def test_perturb_noise_is_added_to_the_window_in_front_of_the_kernels():
    """noise in "perturb" mode: the stage's out-of-place add on the window, then statistics and normalisation of the perturbed window"""
    import makani_amd as ma
    grid, nh, chans = (13, 22), 1, [2, 0]
    pre, win, r = _case(grid, "mean", nh, 2, 0, 0)
    stage = ma.InputNoise(ma.DummyNoiseS2(grid, B, len(chans), num_time_steps=nh + 1, mode="constant_random", seed=9), mode="perturb",
                          perturb_channels=chans, n_history=nh).to(DEV)
    pre.noise_stage = stage
    pre.update_internal_state(replace_state=True)
    field = stage.input_noise.state.detach().clone()
    before = win.clone()
    with torch.no_grad():
        out = pre.assemble(win)
    assert torch.equal(win, before)          # out of place
    w5 = r["win"].reshape(B, nh + 1, C, *grid).clone()
    w5[:, :, chans] += field.double().cpu()
    want, mu, sigma = ref.assemble(w5.flatten(1, 2).float().double(), r["unp"], None, None, nh + 1, "mean", r["q"], r["wt"])
    e = ref.rel(out, want)
    print(f"perturb: {e:.1e}")
    assert tuple(out.shape) == (B, 2 * (C + 2), *grid) and bool(field.any()) and e <= 1e-6


def test_forward_and_backward_replay_from_a_captured_graph():
    import makani_amd as ma
    grid = (33, 64)
    pre, win, r = _case(grid, "mean", 2, 2, 1, 5)
    cin = 3 * (C + 3) + 5
    torch.manual_seed(2)
    net = ma.PointwiseConv(cin, C).to(DEV)
    g_out = torch.randn((B, C, *grid), device=DEV)

    def run(x):
        y = pre.finish(net(pre.assemble(x)))
        return y, torch.autograd.grad((y * g_out).sum(), [x, net.weight])

    run(win.clone().requires_grad_(True))          # warms up outside the capture
    static = win.clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            y, grads = run(static)
    torch.cuda.current_stream().wait_stream(stream)
    gen = torch.Generator().manual_seed(99)
    for _ in range(2):
        fresh = win + (0.5 * torch.randn(win.shape, generator=gen)).to(DEV)
        with torch.no_grad():
            static.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        want, gw = run(fresh.clone().requires_grad_(True))
        assert torch.equal(y, want) and all(torch.equal(a, b) for a, b in zip(grads, gw))


# ---- the rollout wrapper ---------------------------------------------------------------------------------------------------
class _Conv1x1(torch.nn.Linear):
    def forward(self, x):
        return super().forward(x.movedim(1, -1)).movedim(-1, 1)


def _rollout_setup(push_forward=False, checkpoint=False):
    import makani_amd as ma
    grid, nh, nf, U, N = (13, 22), 1, 2, 2, 1
    T = nh + 1
    gen = torch.Generator().manual_seed(11)
    win = _field((B, T, C, *grid), 3.0, gen, 2).flatten(1, 2)
    unp = _field((B, T, U, *grid), 3.0, gen, 2)
    tar = _field((B, nf + 1, U, *grid), 3.0, gen, 2)
    bias = 0.2 * torch.randn((1, C, *grid), generator=gen)

    def process():
        return ma.DummyNoiseS2(grid, B, N, num_time_steps=T, mode="constant_random", seed=21).to(DEV)

    pre = ma.Preprocessor2D(img_shape=grid, n_history=nh, history_normalization_mode="mean", bias_correction=bias,
                            input_noise=ma.InputNoise(process(), n_history=nh)).to(DEV)
    torch.manual_seed(4)
    net = torch.nn.Sequential(_Conv1x1(T * (C + U + N), 8), torch.nn.Tanh(), _Conv1x1(8, C))
    wrap = ma.MultiStepWrapper(net, n_future=nf, n_history=nh, push_forward=push_forward, multistep_checkpoint=checkpoint,
                               preprocessor=pre).to(DEV)
    wrap.train()
    pre.cache_unpredicted_features(None, None, unp.to(DEV), tar.to(DEV))
    # the fields the wrapper will see: a twin process of the same seed, advanced as the wrapper advances its own
    twin, noises = process(), []
    twin.update(replace_state=True)
    for step in range(nf + 1):
        noises.append(twin().detach().clone().double().cpu())
        twin.update()
    r = dict(win=win.double(), unp=unp.double(), tar=tar.double(), bias=bias[0].double(), noises=noises, q=ref.quad_weights(*grid),
             wt=ref.time_weights("mean", nh), T=T, nf=nf)
    return wrap, net, win.to(DEV), r


def _run_rollout(push_forward=False, checkpoint=False):
    import copy
    wrap, net, win, r = _rollout_setup(push_forward, checkpoint)
    net64 = copy.deepcopy(net).double().cpu()
    win = win.requires_grad_(True)
    out = wrap(win)
    gen = torch.Generator().manual_seed(8)
    rnd = torch.randn(out.shape, generator=gen)
    (out * rnd.to(DEV)).sum().backward()
    w64 = r["win"].clone().requires_grad_(True)
    want = ref.rollout(net64, w64, r["unp"], r["tar"], r["noises"], None, r["bias"], r["T"], "mean", r["q"], r["wt"], r["nf"],
                       push_forward=push_forward)
    (want * rnd.double()).sum().backward()
    return wrap, out, win, net, want, w64, net64


@pytest.mark.parametrize("checkpoint", [False, True], ids=["plain", "checkpointed"])
def test_three_step_rollout_against_the_restatement(checkpoint):
    wrap, out, win, net, want, w64, net64 = _run_rollout(checkpoint=checkpoint)
    assert tuple(out.shape) == (B, 3 * C, 13, 22)
    e_out, e_win = ref.rel(out, want), ref.rel(win.grad, w64.grad)
    e_par = max(ref.rel(p.grad, p64.grad) for p, p64 in zip(net.parameters(), net64.parameters()))
    print(f"rollout checkpoint={checkpoint}: output {e_out:.1e} window gradient {e_win:.1e} parameter gradients {e_par:.1e}")
    assert max(e_out, e_win, e_par) <= 1e-5
    # the cached unpredicted input has moved two steps on
    assert torch.equal(wrap.preprocessor.unpredicted_inp_train, wrap.preprocessor.unpredicted_tar_train[:, 0:2])
    if checkpoint:
        _, out0, win0, net0, _, _, _ = _run_rollout(checkpoint=False)
        assert torch.equal(out, out0) and torch.equal(win.grad, win0.grad)
        assert all(torch.equal(p.grad, p0.grad) for p, p0 in zip(net.parameters(), net0.parameters()))


def test_push_forward_mode_gives_no_gradient_into_the_window():
    wrap, out, win, net, want, w64, net64 = _run_rollout(push_forward=True)
    assert win.grad is None or not bool(win.grad.any())
    assert w64.grad is None or not bool(w64.grad.any())
    e_out = ref.rel(out, want)
    e_par = max(ref.rel(p.grad, p64.grad) for p, p64 in zip(net.parameters(), net64.parameters()))
    print(f"push-forward rollout: output {e_out:.1e} parameter gradients {e_par:.1e}")
    assert max(e_out, e_par) <= 1e-5


def test_single_step_wrapper_and_eval_path():
    import makani_amd as ma
    pre, win, r = _case((13, 22), "mean", 1, 2, 0, 5)
    torch.manual_seed(4)
    net = _Conv1x1(2 * (C + 2) + 5, C).to(DEV)
    single = ma.SingleStepWrapper(net, preprocessor=pre)
    multi = ma.MultiStepWrapper(net, n_future=2, n_history=1, preprocessor=pre)
    single.eval(), multi.eval()
    pre.cache_unpredicted_features(None, None, pre.unpredicted_inp_train, pre.unpredicted_tar_train)          # the eval cache
    with torch.no_grad():
        y1, y2 = single(win), multi(win)
    x, mu, sigma = _ref_assemble(r, "mean")
    want = ref.finish(net.double().cpu()(x), r["bias"], mu, sigma)
    e = ref.rel(y1, want)
    print(f"single step, eval: {e:.1e}")
    assert torch.equal(y1, y2) and tuple(y1.shape) == (B, C, 13, 22) and e <= 1e-5
