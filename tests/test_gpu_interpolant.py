"""The stochastic-interpolant stepper (csrc/interpolant.hip behind ``makani_amd.interpolant``) on the GPU against the fp64
restatement tests/_interp_ref.py, itself pinned against the reference's class by tests/test_interpolant.py.

Gates (those of tests/test_gpu_constraints.py).  f32: 2 x the reference's own fp32 error + one fp32 ulp of the largest magnitude of
the compared tensor.  For a fixture case the reference's error is the recorded ``err32_*`` (the class's own fp32 CPU run against
its double run); for inputs generated here it is the distance between the restated formula in fp32 torch and in fp64 on those very
inputs.  bf16: the result equals the fp64 restatement of the bf16 inputs, rounded to bf16, or is its neighbour.  Copied slots are
compared with torch.equal.  Neither gate is taken from the code under test.

Grids: 9 x 17 (HW = 153, odd: one pixel per thread and a single partial chunk) and 34 x 64 (HW = 2176: the 16-byte path;
mk_plane_chunks cuts it into 3 chunks of 728, 728 and 720 pixels — 33 x 64 = 3 x 704 would leave no tail), plus an x0 that starts
one element into its storage (misaligned: one pixel per thread at a HW that is a multiple of 4).  At those sizes a thread of the
16-byte path makes one pass of its pixel loop; 180 x 368 (64 chunks of 1036 pixels) makes some take a second one.  The gradient
test runs on both grids, so both instantiations of the backward kernel are launched.  bf16 sampler steps are gated from the number
formats alone (the docstrings of those tests say how)."""
import pytest
import torch

import _interp_ref as ref
from _preproc_ref import seeded
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ref.load_cases(load_golden("interpolant.npz"))
NAMES = sorted(CASES)
GRIDS = [(9, 17), (34, 64)]
B, C, U, ST, NS = 2, 3, 2, 2, 3


class Stub(torch.nn.Module):
    """Conv2d(inp_chans, C, 1) that records what it is called with; the time-aware form hands it the time, which it ignores"""

    def __init__(self, cin, seed, scale=(0.3, 0.1)):
        super().__init__()
        self.conv = torch.nn.Conv2d(cin, C, 1)
        with torch.no_grad():
            self.conv.weight.copy_(scale[0] * seeded(self.conv.weight.shape, seed))
            self.conv.bias.copy_(scale[1] * seeded(self.conv.bias.shape, seed + 1))
        self.calls = []

    def forward(self, x, s=None):
        self.calls.append((x.detach(), None if s is None else s.detach()))
        return self.conv(x)


class InjectedNoiseOnly(torch.nn.Module):
    """stands in for the noise module on the 9 x 17 grid (the package's FFT takes even longitude counts only): every draw of the
    tests on that grid is injected as a field, so the module is only ever asked to resize"""

    def update(self, replace_state=False, batch_size=None, innovation=None):
        pass

    def forward(self, update_internal_state=False):
        raise AssertionError("the noise of this test is injected")


def wrapper(grid, xu, static, *, seed=50, scale=(0.3, 0.1), n=B, **kw):
    """the wrapper under test around the stub, the features cached for both modes"""
    import makani_amd as ma
    ta = kw.get("time_aware", False)
    cin = 2 * C + (0 if xu is None else xu.shape[2]) + (0 if static is None else static.shape[1]) + (0 if ta else 1)
    noise = InjectedNoiseOnly() if grid[1] % 2 else ma.IsotropicGaussianRandomFieldS2(grid, n, C)
    w = ma.StochasticInterpolantWrapper(Stub(cin, seed, scale), ma.Preprocessor2D(img_shape=grid, static_features=static), noise,
                                        n_pred_chans=C, **kw).to(DEV)
    for mode in (True, False):
        w.train(mode)
        w.preprocessor.cache_unpredicted_features(None, None, None if xu is None else xu.to(DEV), None)
    return w


def gate32(err32, want):
    return 2.0 * float(err32) + ref.ulp32(want)


def bf16_steps(a, b):
    """distance of two bf16 tensors in representable values"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs().max().item()


# ---- 1. the training assemble --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_training_call_against_the_fixture(case):
    c = CASES[case]
    m = c["meta"]
    x0, x1, xu, static = ref.case_inputs(c)
    cin = 2 * C + m["U"] + m["St"] + (0 if m["time_aware"] else 1)
    w = wrapper((m["H"], m["W"]), xu, static, seed=m["seeds"]["net"], scale=m["net_scale"], noise_epsilon=m["eps"], use_foellmer=m["foellmer"],
                antithetic_sampling=m["antithetic"], time_aware=m["time_aware"]).train()
    assert w.model.model.conv.in_channels == cin
    pred, drift = w(x0.to(DEV), x1.to(DEV), n_samples=m["n_samples"], s=c["s_draw"], noise=c["z"].unsqueeze(0).to(DEV))
    (X, s_seen), = w.model.model.calls
    X, drift, Sp = X.cpu(), drift.cpu(), c["s"].shape[1]
    assert X.dtype == torch.float32 and drift.dtype == torch.float32 and tuple(X.shape) == (m["B"] * Sp, cin, m["H"], m["W"])
    assert tuple(pred.shape) == tuple(drift.shape) == (m["B"] * Sp, C, m["H"], m["W"])
    want_X, _ = ref.assemble(x0, x1, c["z"], c["s"], None if xu is None else xu[:, 0], None if static is None else static[0], m["eps"],
                             has_s=not m["time_aware"])
    assert torch.equal(X[:, :C], want_X[:, :C].float()) and torch.equal(X[:, 2 * C:], want_X[:, 2 * C:].float())
    if m["time_aware"]:
        assert torch.equal(s_seen.cpu(), c["s"].flatten().unsqueeze(1))
    e_x, e_d = (X[:, C:2 * C].double() - c["x64"]).abs().max().item(), (drift.double() - c["drift64"]).abs().max().item()
    g_x, g_d = gate32(c["err32_x"], c["x64"]), gate32(c["err32_drift"], c["drift64"])
    print(f"{case}: x slot {e_x:.3e} (gate {g_x:.3e})  drift {e_d:.3e} (gate {g_d:.3e})")
    assert e_x <= g_x and e_d <= g_d


def _generated(grid, bf16=False):
    """inputs of the generated cases, shared by the tests below: s holds exactly 0 and exactly 1 (and, mirrored, 1 and 0)"""
    H, W = grid
    x0, x1, z = (seeded((B, C, H, W), 100 + k).float() for k in range(3))
    xu, static = seeded((B, 1, U, H, W), 103).float(), seeded((1, ST, H, W), 104).float()
    s_draw = torch.tensor([[0.0, 0.3137, 1.0], [0.5, 0.0625, 0.9871]], dtype=torch.float32)
    if bf16:
        x0, x1 = x0.bfloat16(), x1.bfloat16()
    return x0, x1, z, xu, static, s_draw


@pytest.mark.parametrize("eps", [1.0, 0.7])
@pytest.mark.parametrize("grid", GRIDS)
def test_training_assemble_on_generated_inputs_f32(grid, eps):
    from makani_amd.ops import si_assemble
    x0, x1, z, xu, static, s_draw = _generated(grid)
    s = torch.cat([s_draw, 1.0 - s_draw], dim=1)          # antithetic pairs: S' = 6
    want_X, want_D = ref.assemble(x0, x1, z, s, xu[:, 0], static[0], eps)
    X32, D32 = ref.assemble(x0, x1, z, s, xu[:, 0], static[0], eps, dtype=torch.float32)
    X, D = si_assemble(x0.to(DEV), x1.to(DEV), z.to(DEV), s.to(DEV), xu[:, 0].to(DEV), static[0].to(DEV), eps)
    X, D = X.cpu(), D.cpu()
    assert X.dtype == torch.float32 and tuple(X.shape) == (B * 2 * NS, 2 * C + U + ST + 1, *grid) and tuple(D.shape) == (B * 2 * NS, C, *grid)
    assert torch.equal(X[:, :C], want_X[:, :C].float()) and torch.equal(X[:, 2 * C:], want_X[:, 2 * C:].float())
    wx = want_X[:, C:2 * C]
    e_x, e_d = (X[:, C:2 * C].double() - wx).abs().max().item(), (D.double() - want_D).abs().max().item()
    g_x = gate32((X32[:, C:2 * C].double() - wx).abs().max(), wx)
    g_d = gate32((D32.double() - want_D).abs().max(), want_D)
    print(f"{grid} eps {eps}: x slot {e_x:.3e} (gate {g_x:.3e})  drift {e_d:.3e} (gate {g_d:.3e})")
    assert e_x <= g_x and e_d <= g_d
    # without features and without the s plane (the time-aware layout): the slots that remain
    X2, D2 = si_assemble(x0.to(DEV), x1.to(DEV), z.to(DEV), s.to(DEV), None, None, eps, has_s=False)
    assert tuple(X2.shape) == (B * 2 * NS, 2 * C, *grid) and torch.equal(X2.cpu(), X[:, :2 * C]) and torch.equal(D2.cpu(), D)


@pytest.mark.parametrize("grid", GRIDS)
def test_training_assemble_bf16(grid):
    """bf16 x0 / x1 and a bf16 network input (``input_dtype=torch.bfloat16``): X is the fp64 restatement of the bf16 inputs rounded
    to bf16, or its neighbour; the drift target stays float32 under the f32 gate"""
    eps = 0.7
    x0, x1, z, xu, static, s_draw = _generated(grid, bf16=True)
    w = wrapper(grid, xu, static, noise_epsilon=eps, antithetic_sampling=True, input_dtype=torch.bfloat16)
    w.train()
    w.model.model.to(torch.bfloat16)
    pred, D = w(x0.to(DEV), x1.to(DEV), n_samples=NS, s=s_draw, noise=z.unsqueeze(0).to(DEV))
    (X, _), = w.model.model.calls
    X, D = X.cpu(), D.cpu()
    s = torch.cat([s_draw, 1.0 - s_draw], dim=1)
    want_X, want_D = ref.assemble(x0.double(), x1.double(), z, s, xu[:, 0], static[0], eps)
    _, D32 = ref.assemble(x0.float(), x1.float(), z, s, xu[:, 0], static[0], eps, dtype=torch.float32)
    assert X.dtype == torch.bfloat16 and D.dtype == torch.float32
    assert torch.equal(X[:, :C], want_X[:, :C].bfloat16()) and torch.equal(X[:, 2 * C:], want_X[:, 2 * C:].bfloat16())
    steps = bf16_steps(X[:, C:2 * C], want_X[:, C:2 * C].bfloat16())
    e_d, g_d = (D.double() - want_D).abs().max().item(), gate32((D32.double() - want_D).abs().max(), want_D)
    print(f"{grid}: bf16 steps of the x slot {steps}; drift {e_d:.3e} (gate {g_d:.3e})")
    assert steps <= 1 and e_d <= g_d


def test_misaligned_x0_takes_the_one_pixel_path_with_the_same_result():
    from makani_amd.ops import si_assemble, si_step
    grid = GRIDS[1]
    x0, x1, z, xu, static, s_draw = (t.to(DEV) for t in _generated(grid))
    buf = torch.zeros(x0.numel() + 1, device=DEV)
    view = buf[1:].view(x0.shape)
    view.copy_(x0)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and x0.data_ptr() % 16 == 0
    s = torch.cat([s_draw, 1.0 - s_draw], dim=1)
    for a, b in zip(si_assemble(view, x1, z, s, xu[:, 0], static[0], 0.7), si_assemble(x0, x1, z, s, xu[:, 0], static[0], 0.7)):
        assert torch.equal(a, b)
    coef = (0.75, 0.5, -0.25, 0.3)
    args = (x1, x0, z, xu[:, 0], static[0], coef, 0.5)
    assert torch.equal(si_step(view, *args), si_step(x0, *args))
    assert torch.equal(si_step(view, *args, last=True), si_step(x0, *args, last=True))


# ---- 2. the sampler ------------------------------------------------------------------------------------------------------------
def _sampler_case(grid, eps, foellmer, steps, time_aware=False):
    H, W = grid
    x0, _, _, xu, static, _ = _generated(grid)
    noises = seeded((steps, B, C, H, W), 200 + steps).float()
    w = wrapper(grid, xu, static, noise_epsilon=eps, use_foellmer=foellmer, time_aware=time_aware).eval()
    conv = w.model.model.conv

    def restated(dtype):
        net = ref.stub(conv.weight.detach().cpu(), conv.bias.detach().cpu(), dtype)
        return ref.sampler(net, x0, xu[:, 0], static[0], list(noises), steps, eps, foellmer, time_aware=time_aware, dtype=dtype)

    return w, x0, noises, restated


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("foellmer", [False, True])
@pytest.mark.parametrize("eps", [1.0, 0.7])
@pytest.mark.parametrize("grid", GRIDS)
def test_sampler_against_the_restatement(grid, eps, foellmer, steps):
    w, x0, noises, restated = _sampler_case(grid, eps, foellmer, steps)
    want = restated(torch.float64)
    gate = gate32((restated(torch.float32).double() - want).abs().max(), want)
    with torch.no_grad():
        y = w(x0.to(DEV), n_steps=steps, noise=noises.to(DEV)).cpu()
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, C, *grid)
    calls = w.model.model.calls
    assert len(calls) == steps and all(tuple(x.shape) == (B, 2 * C + U + ST + 1, *grid) for x, _ in calls)
    for i, (x, _) in enumerate(calls):          # the copied slots of every network input, and the time plane
        x = x.cpu()
        assert torch.equal(x[:, :C], x0) and torch.equal(x[:, 2 * C:2 * C + U], _generated(grid)[3][:, 0])
        assert torch.equal(x[:, -1], torch.full((B, *grid), float(torch.linspace(0, 1, steps + 1)[i])))
    assert torch.equal(calls[0][0][:, C:2 * C].cpu(), x0)
    e = (y.double() - want).abs().max().item()
    print(f"{grid} eps {eps} foellmer {foellmer} n_steps {steps}: {e:.3e} (gate {gate:.3e})")
    assert e <= gate


def test_sampler_against_the_fixture():
    """the recorded samplers (the reference's own float64 run, its static planes at B = 1) under the recorded error"""
    for case in NAMES:
        c = CASES[case]
        m = c["meta"]
        x0, _, xu, static = ref.case_inputs(c)
        n = m["sampler_B"]
        w = wrapper((m["H"], m["W"]), None if xu is None else xu[:n], static, seed=m["seeds"]["net"], n=n, noise_epsilon=m["eps"],
                    use_foellmer=m["foellmer"], time_aware=m["time_aware"]).eval()
        for steps in m["n_steps"]:
            with torch.no_grad():
                y = w(x0[:n].to(DEV), n_steps=steps, noise=c[f"noise_n{steps}"].to(DEV)).cpu()
            want = c[f"y64_n{steps}"]
            e, gate = (y.double() - want).abs().max().item(), gate32(c[f"err32_y_n{steps}"], want)
            print(f"{case} n_steps {steps}: {e:.3e} (gate {gate:.3e})")
            assert e <= gate, (case, steps)


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_gradients_of_the_three_step_foellmer_sampler(grid):
    """9 x 17 backpropagates through the one-pixel instantiation of mk_si_step_bwd, 34 x 64 through the 16-byte one"""
    eps, steps = 0.7, 3
    w, x0, noises, _ = _sampler_case(grid, eps, True, steps)
    conv = w.model.model.conv
    x, _, _, xu, static, _ = _generated(grid)
    r = seeded((B, C, *grid), 300)

    def restated(dtype):
        wt, bs = conv.weight.detach().cpu().to(dtype).requires_grad_(True), conv.bias.detach().cpu().to(dtype).requires_grad_(True)
        xi = x0.to(dtype).requires_grad_(True)
        net = lambda t, s=None: torch.nn.functional.conv2d(t, wt, bs)
        y = ref.sampler(net, xi, xu[:, 0], static[0], list(noises), steps, eps, True, dtype=dtype)
        return torch.autograd.grad((y * r.to(dtype)).sum(), [xi, wt, bs])

    want, low = restated(torch.float64), restated(torch.float32)
    xi = x0.to(DEV).requires_grad_(True)
    y = w(xi, n_steps=steps, noise=noises.to(DEV))
    got = torch.autograd.grad((y * r.float().to(DEV)).sum(), [xi, conv.weight, conv.bias])
    for name, g, wv, lv in zip(("inp", "weight", "bias"), got, want, low):
        e, gate = (g.cpu().double() - wv).abs().max().item(), gate32((lv.double() - wv).abs().max(), wv)
        print(f"gradient w.r.t. {name}: {e:.3e} (gate {gate:.3e})")
        assert g.shape == wv.shape and e <= gate, name


# ---- 3b. a second pass of the pixel loop, bf16 steps, injected innovations -----------------------------------------------------
# HW = 66240 > 64 x 1024: mk_plane_chunks stops at 64 chunks, here of 1036 pixels (the last of 972), so the threads that own the
# first 12 pixels of a chunk take a second pass of the 16-byte loop (256 threads x 4 pixels per pass)
BIG = (180, 368)
COEF = (0.4375, 0.625, -0.3125, 0.46875)          # (cx, cb, c0, cn), exact in float32
S_NEXT = 0.75


def _step_case(grid, dtype):
    """one sampler step through SiStepFn, forward and backward: leaves, result, gradients and the fp64 statement of both"""
    from makani_amd.ops import SiStepFn
    H, W = grid
    cin = 2 * C + U + ST + 1
    prev, g = seeded((B, cin, H, W), 500).float().to(dtype), seeded((B, cin, H, W), 501).float().to(dtype)
    b, x0 = seeded((B, C, H, W), 502).float().to(dtype), seeded((B, C, H, W), 503).float().to(dtype)
    z, xu, static = seeded((B, C, H, W), 504).float(), seeded((B, U, H, W), 505).float(), seeded((ST, H, W), 506).float()
    pd, bd, x0d = (t.to(DEV).requires_grad_(True) for t in (prev, b, x0))
    out = SiStepFn.apply(pd[:, C:2 * C], bd, x0d, z.to(DEV), xu.to(DEV), static.to(DEV), COEF, S_NEXT, False, True, dtype)
    gp, gb, g0 = torch.autograd.grad(out, [pd, bd, x0d], g.to(DEV))
    cx, cb, c0, cn = COEF
    terms = [cx * prev[:, C:2 * C].double(), cb * b.double(), c0 * x0.double(), cn * z.double()]
    g0s, g1 = g[:, :C].double(), g[:, C:2 * C].double()
    want = dict(x=sum(terms), S=sum(t.abs() for t in terms), gx=cx * g1, gb=cb * g1, gx0=g0s + c0 * g1, S0=g0s.abs() + (c0 * g1).abs(),
                copies=ref.net_input(x0.double(), sum(terms), xu, static, torch.full((B,), S_NEXT, dtype=torch.float64)))
    return (prev, b, x0, z, g), out.detach().cpu(), (gp.cpu(), gb.cpu(), g0.cpu()), want


def test_a_thread_takes_a_second_pass_of_the_pixel_loop():
    from makani_amd.ops import si_assemble
    H, W = BIG
    x0, x1, z = (seeded((B, C, H, W), 510 + k).float() for k in range(3))
    xu, static = seeded((B, U, H, W), 513).float(), seeded((ST, H, W), 514).float()
    s = torch.tensor([[0.0, 0.3137], [1.0, 0.5]], dtype=torch.float32)
    want_X, want_D = ref.assemble(x0, x1, z, s, xu, static, 0.7)
    X32, D32 = ref.assemble(x0, x1, z, s, xu, static, 0.7, dtype=torch.float32)
    X, D = (t.cpu() for t in si_assemble(x0.to(DEV), x1.to(DEV), z.to(DEV), s.to(DEV), xu.to(DEV), static.to(DEV), 0.7))
    assert torch.equal(X[:, :C], want_X[:, :C].float()) and torch.equal(X[:, 2 * C:], want_X[:, 2 * C:].float())
    wx = want_X[:, C:2 * C]
    e_x, e_d = (X[:, C:2 * C].double() - wx).abs().max().item(), (D.double() - want_D).abs().max().item()
    g_x, g_d = gate32((X32[:, C:2 * C].double() - wx).abs().max(), wx), gate32((D32.double() - want_D).abs().max(), want_D)
    print(f"{BIG}: x slot {e_x:.3e} (gate {g_x:.3e})  drift {e_d:.3e} (gate {g_d:.3e})")
    assert e_x <= g_x and e_d <= g_d
    # one sampler step and its backward at the same size; the single products of the backward are exact in either arithmetic
    (prev, b, x0s, zs, g), out, (gp, gb, g0), want = _step_case(BIG, torch.float32)
    cx, cb, c0, cn = COEF
    x32 = cx * prev[:, C:2 * C] + cb * b + c0 * x0s + cn * zs
    assert torch.equal(out[:, :C], x0s) and torch.equal(out[:, 2 * C:], want["copies"][:, 2 * C:].float())
    e, gate = (out[:, C:2 * C].double() - want["x"]).abs().max().item(), gate32((x32.double() - want["x"]).abs().max(), want["x"])
    assert e <= gate, (e, gate)
    assert torch.equal(gp[:, C:2 * C], cx * g[:, C:2 * C]) and not bool(gp[:, :C].any()) and not bool(gp[:, 2 * C:].any())
    assert torch.equal(gb, cb * g[:, C:2 * C])
    e0 = (g0.double() - want["gx0"]).abs().max().item()
    gate0 = gate32(((g[:, :C] + c0 * g[:, C:2 * C]).double() - want["gx0"]).abs().max(), want["gx0"])
    print(f"{BIG}: step {e:.3e} (gate {gate:.3e})  g_x0 {e0:.3e} (gate {gate0:.3e})")
    assert e0 <= gate0


@pytest.mark.parametrize("grid", GRIDS)
def test_bf16_step_forward_and_backward(grid):
    """bf16 x, b, x0, gradient and network input.  Gate, per element, from the number formats alone: the kernel sums at most four
    products in fp32 (error at most 5 x 2^-24 of the sum of their magnitudes, S) and rounds once to bf16 (half a step, at most
    2^-8 of the value): |got - want| <= 2^-8 (|want| + d) + d, d = 5 x 2^-24 S."""
    (prev, b, x0, z, g), out, (gp, gb, g0), want = _step_case(grid, torch.bfloat16)
    assert out.dtype == torch.bfloat16 and all(t.dtype == torch.bfloat16 for t in (gp, gb, g0))

    def within(got, wv, S):
        d = 5.0 * 2.0 ** -24 * S
        return bool(((got.double() - wv).abs() <= 2.0 ** -8 * (wv.abs() + d) + d).all())

    assert torch.equal(out[:, :C], x0) and torch.equal(out[:, 2 * C:], want["copies"][:, 2 * C:].bfloat16())
    assert within(out[:, C:2 * C], want["x"], want["S"])
    assert within(gp[:, C:2 * C], want["gx"], want["gx"].abs()) and not bool(gp[:, :C].any()) and not bool(gp[:, 2 * C:].any())
    assert within(gb, want["gb"], want["gb"].abs()) and within(g0, want["gx0"], want["S0"])


def test_bf16_sampler_stays_within_the_propagated_rounding_bound():
    """``input_dtype=torch.bfloat16`` around a bf16 stub, three Foellmer steps, against the fp64 restatement with the stub's (bf16)
    weights.  The bound follows the bf16 roundings (u = 2^-8 of the value) through the loop, with magnitudes from the fp64 trajectory:
    every slot of the network input is stored in bf16 (error u max|slot|, the x slot on top of the carried error E); the stub's
    output errs by its rows' |W| applied to the slot errors plus u max|b| for its own bf16 result (it accumulates in fp32);
    the kernel reads x0, z in float32 and the carried x from its bf16 slot, so E' = |cx| (E + u max|x|) + |cb| E_b, and the last
    step writes float32.  1e-6 covers the float32 arithmetic and the float32 step times."""
    grid, eps, steps = GRIDS[1], 0.7, 3
    x0, _, _, xu, static, _ = _generated(grid)
    noises = seeded((steps, B, C, *grid), 230).float()
    w = wrapper(grid, xu, static, noise_epsilon=eps, use_foellmer=True, input_dtype=torch.bfloat16).eval()
    conv = w.model.model.conv.to(torch.bfloat16)
    Wm, bias = conv.weight.detach().cpu().double().reshape(C, -1), conv.bias.detach().cpu().double()
    net = ref.stub(Wm, bias)
    want = ref.sampler(net, x0, xu[:, 0], static[0], list(noises), steps, eps, True)
    u = 2.0 ** -8
    st = torch.linspace(0, 1, steps + 1, dtype=torch.float32)
    ds, st = (st[1:] - st[:-1]).double().tolist(), st.double().tolist()
    slot_max = [float(x0.abs().max())] * C + [0.0] * C + [float(xu[:, 0, k].abs().max()) for k in range(U)] + \
               [float(static[0, k].abs().max()) for k in range(ST)] + [1.0]
    x, E = x0.double(), 0.0
    for i in range(steps):
        xin = ref.net_input(x0.double(), x, xu[:, 0], static[0], torch.full((B,), st[i], dtype=torch.float64))
        b = net(xin)
        err = torch.tensor([u * m for m in slot_max], dtype=torch.float64)
        err[C:2 * C] = E + u * float(x.abs().max())
        E_b = float((Wm.abs() @ err).max()) + u * float(b.abs().max())
        cx, cb, c0, cn = ref.generic_coefficients(st[i], ds[i], eps, True, i == 0)
        E = abs(cx) * (E + (u * float(x.abs().max()) if i > 0 else 0.0)) + abs(cb) * E_b
        x = cx * x + cb * b + c0 * x0.double() + cn * noises[i].double()
    assert float((x - want).abs().max()) <= 1e-6          # the trajectory above is the restated sampler
    with torch.no_grad():
        y = w(x0.to(DEV), n_steps=steps, noise=noises.to(DEV)).cpu()
    calls = w.model.model.calls
    assert y.dtype == torch.float32 and len(calls) == steps and all(t.dtype == torch.bfloat16 for t, _ in calls)
    e = (y.double() - want).abs().max().item()
    print(f"bf16 sampler: {e:.3e} (bound {E + 1e-6:.3e}, largest value {float(want.abs().max()):.2f})")
    assert e <= E + 1e-6


def test_injected_innovations_go_through_the_noise_module():
    """``noise=`` as innovations of the spectral state (K, B, 1, C, L, M, 2): the same result as injecting the fields that a second
    module of the same kind synthesises from them, in training (K = 1) and in the sampler (K = n_steps)"""
    import makani_amd as ma
    grid, steps = GRIDS[1], 2
    x0, x1, _, xu, static, s_draw = _generated(grid)
    w = wrapper(grid, xu, static, noise_epsilon=0.7, use_foellmer=True)
    other = ma.IsotropicGaussianRandomFieldS2(grid, B, C).to(DEV)
    xi = seeded((steps, B, 1, C, other.lmax, other.mmax, 2), 240).float().to(DEV)
    fields = []
    for k in range(steps):
        other.update(innovation=xi[k])
        fields.append(other().squeeze(1).clone())
    fields = torch.stack(fields)
    assert tuple(fields.shape) == (steps, B, C, *grid) and bool(fields.abs().max() > 0.1)
    w.eval()
    with torch.no_grad():
        assert torch.equal(w(x0.to(DEV), n_steps=steps, noise=xi), w(x0.to(DEV), n_steps=steps, noise=fields))
    w.train()
    a = w(x0.to(DEV), x1.to(DEV), n_samples=NS, s=s_draw, noise=xi[:1])
    b = w(x0.to(DEV), x1.to(DEV), n_samples=NS, s=s_draw, noise=fields[:1])
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


# ---- 4. the time-aware form ------------------------------------------------------------------------------------------------
def test_time_aware_network_receives_the_input_and_the_time():
    grid = GRIDS[0]
    x0, x1, z, xu, static, s_draw = _generated(grid)
    w = wrapper(grid, xu, static, noise_epsilon=0.7, antithetic_sampling=True, time_aware=True)
    import makani_amd as ma
    assert isinstance(w.model, ma.TimeAwareInterpolationWrapper) and w.model.model.conv.in_channels == 2 * C + U + ST
    w.train()
    pred, drift = w(x0.to(DEV), x1.to(DEV), n_samples=NS, s=s_draw, noise=z.unsqueeze(0).to(DEV))
    (X, s_seen), = w.model.model.calls
    s = torch.cat([s_draw, 1.0 - s_draw], dim=1)
    assert tuple(X.shape) == (B * 2 * NS, 2 * C + U + ST, *grid) and torch.equal(s_seen.cpu(), s.flatten().unsqueeze(1))
    want_X, want_D = ref.assemble(x0, x1, z, s, xu[:, 0], static[0], 0.7, has_s=False)
    assert torch.equal(X[:, :C].cpu(), want_X[:, :C].float()) and torch.equal(X[:, 2 * C:].cpu(), want_X[:, 2 * C:].float())
    assert tuple(pred.shape) == tuple(drift.shape) == (B * 2 * NS, C, *grid)
    w.eval()
    w.model.model.calls.clear()
    steps = 3
    w2, _, noises, restated = _sampler_case(grid, 0.7, True, steps, time_aware=True)
    with torch.no_grad():
        y = w2(x0.to(DEV), n_steps=steps, noise=noises.to(DEV)).cpu()
    calls = w2.model.model.calls
    assert [tuple(x.shape) for x, _ in calls] == [(B, 2 * C + U + ST, *grid)] * steps
    for i, (_, sv) in enumerate(calls):
        assert torch.equal(sv.cpu(), torch.full((B, 1), float(torch.linspace(0, 1, steps + 1)[i])))
    want = restated(torch.float64)
    assert (y.double() - want).abs().max().item() <= gate32((restated(torch.float32).double() - want).abs().max(), want)


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------
def test_sampler_is_capturable_and_replays_bit_equal_from_a_restored_noise_state():
    grid, steps = GRIDS[1], 2
    x0, _, _, xu, static, _ = _generated(grid)
    w = wrapper(grid, xu, static, noise_epsilon=0.7, use_foellmer=True).eval()
    nm = w.noise_module
    xd = x0.to(DEV)
    nm.update(replace_state=True, batch_size=B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():          # warm-up off the capturing stream
        w._forward_eval(xd, n_steps=steps)
    torch.cuda.current_stream().wait_stream(side)
    state, rng = nm.get_tensor_state(), nm.get_rng_state()
    with torch.no_grad():
        eager = w._forward_eval(xd, n_steps=steps).clone()
    after = nm.get_tensor_state()
    assert not torch.equal(after, state)          # the sampler drew from the module
    nm.set_tensor_state(state)
    nm.set_rng_state(*rng)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = w._forward_eval(xd, n_steps=steps)
    for _ in range(2):
        nm.set_tensor_state(state)
        nm.set_rng_state(*rng)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(nm.get_tensor_state(), after)


# ---- 6. integration --------------------------------------------------------------------------------------------------------
class _Params(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def test_from_params_around_the_sfno_trains_and_samples():
    import makani_amd as ma
    H, W = 33, 64
    params = _Params(img_shape_x=H, img_shape_y=W, img_shape_x_resampled=H, img_shape_y_resampled=W, img_crop_shape_x=H, img_crop_shape_y=W,
                     n_history=0, n_future=0, N_in_predicted_channels=C, N_out_channels=C, N_static_channels=ST, N_dynamic_channels=U,
                     batch_size=B, data_grid_type="equiangular", model_grid_type="equiangular")

    def handle(inp_chans):
        return ma.SphericalFourierNeuralOperatorNet(inp_shape=(H, W), out_shape=(H, W), inp_chans=inp_chans, out_chans=C, scale_factor=2,
                                                    embed_dim=16, num_layers=2, mlp_ratio=2)

    static = seeded((1, ST, H, W), 401).float()
    w = ma.StochasticInterpolantWrapper.from_params(params, handle, noise_epsilon=0.7, use_foellmer=True, antithetic_sampling=True,
                                                    static_features=static).to(DEV)
    xu = seeded((B, 1, U, H, W), 402).float().to(DEV)
    x0, x1 = seeded((B, C, H, W), 403).float().to(DEV), seeded((B, C, H, W), 404).float().to(DEV)
    w.train()
    w.preprocessor.cache_unpredicted_features(None, None, xu, None)
    pred, drift = w(x0, x1, n_samples=NS)
    assert tuple(pred.shape) == tuple(drift.shape) == (B * 2 * NS, C, H, W) and not drift.requires_grad
    torch.nn.functional.mse_loss(pred, drift).backward()
    for name, p in w.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    gen = w.get_internal_rng()
    assert gen is w.rng_gpu and gen.device.type == "cuda"
    w.eval()
    w.preprocessor.cache_unpredicted_features(None, None, xu, None)
    with torch.no_grad():
        y = w(x0, n_steps=2)
    assert tuple(y.shape) == (B, C, H, W) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    with torch.no_grad():
        y2 = w(x0, n_steps=2)
    assert not torch.equal(y, y2)          # fresh noise per call
