"""The inputs of tests/test_gpu_mrollout.py, shared with the CPU check of their conditioning in tests/test_metricshandler.py.

Conditioned as the generators of tests/test_gpu_metrics.py are, so that 1e-5 tests the kernels and not cancellation: members = a
shared field (std 3) + bounded noise (|.| <= 0.35) + the offsets e - (E - 1) / 2; observations spread uniformly over slightly more
than the ensemble's range; on a sixteenth of the points each the observation equals one member, equals two equal members, lies
below all and above all members; the climatology is a smooth field of std 1; weights in [0.5, 1.5).  SSR: the skill of the mean
is about (1.1 (E + 1))^2 / 12, spread / E about E / 12: ``skill - spread / E`` stays well above eps.  ``clamp=True`` is the
dedicated case that does not: the observation EQUALS the member mean (as fp32 forms it), so ``skill - spread / E`` is
``-spread / E``, clearly negative, and the clamp is active by construction.

C = 11 channels; the lists are out of order and non-contiguous: "z500" sits in every list, "sst" in one (RMSE), "w300" is listed
and absent.  One member: the three ensemble lists and the rank-histogram list are empty, as for a deterministic model."""
import torch
import torch.nn.functional as F

GRIDS = [(9, 14), (17, 32), (91, 180)]
B, STEPS, PASSES = 2, 3, 2
NAMES = "u10m t2m sp sst u500 z500 q500 q50 t850 v10m z850".split()
C = len(NAMES)
LISTS = dict(l1_var_names=["z500", "w300", "u10m", "q50"], rmse_var_names=["t2m", "z500", "sst", "u10m"],
             acc_var_names=["z500", "t850", "u500"], crps_var_names=["q500", "z500"], spread_var_names=["z850", "sp", "z500", "t2m"],
             ssr_var_names=["v10m", "z500"], rh_var_names=["z500", "q50"])
DET_LISTS = dict(LISTS, crps_var_names=[], spread_var_names=[], ssr_var_names=[], rh_var_names=[])
f32, bf16 = torch.float32, torch.bfloat16

# (grid, E, dtype of members and target, weight, channel with NaN targets on the second pass | None)
CASES = [(0, 3, f32, False, None), (0, 1, f32, True, "sst"), (0, 32, bf16, False, "z500"), (0, 9, bf16, True, None),
         (1, 2, bf16, True, "z500"), (1, 9, f32, False, "sst"), (1, 32, f32, True, None), (1, 1, bf16, False, None),
         (2, 3, bf16, False, "z500"), (2, 9, f32, True, "sst"), (2, 1, f32, False, "z500"), (2, 2, f32, False, None)]


def case_id(key):
    return "-".join(str(k).replace("torch.", "") for k in key)


def lists(E):
    return LISTS if E > 1 else DET_LISTS


def scale():
    return torch.linspace(0.5, 3.0, C)


def climatology(grid):
    gen = torch.Generator().manual_seed(7 + grid)
    s = F.interpolate(torch.randn(C, 1, 4, 8, generator=gen), size=GRIDS[grid], mode="bilinear", align_corners=True)
    return s.reshape(1, C, *GRIDS[grid])


def call_inputs(key, call, clamp=False):
    """(prediction, target, weight | None) of update number ``call`` of a case, in the case's dtype (weights fp32); the target of
    the second pass holds NaN on a third of the points of the named channel of sample 1"""
    grid, E, dt, with_w, nan_name = key
    img = GRIDS[grid]
    gen = torch.Generator().manual_seed(1000 * grid + 31 * E + call)
    base = 3.0 * torch.randn(B, C, *img, generator=gen)
    f = (base.unsqueeze(1) + 0.7 * (torch.rand(B, E, C, *img, generator=gen) - 0.5)
         + (torch.arange(E) - 0.5 * (E - 1)).reshape(1, E, 1, 1, 1)).to(dt).float()          # the values the kernel sees
    o = base + 1.1 * (E + 1) * (torch.rand(B, C, *img, generator=gen) - 0.5)
    kind = (torch.arange(img[0] * img[1]) % 16).reshape(img)
    if E >= 2:
        f[:, 1] = torch.where(kind == 1, f[:, 0], f[:, 1])
    o = torch.where(kind == 0, f[:, E // 2], o)
    o = torch.where(kind == 1, f[:, 0], o)
    o = torch.where(kind == 2, f.min(dim=1).values - 1.0, o)
    o = torch.where(kind == 3, f.max(dim=1).values + 1.0, o)
    if clamp:
        o = f.mean(dim=1)
    o = o.to(dt)
    w = (torch.rand(B, C, *img, generator=gen) + 0.5) if with_w else None
    if nan_name is not None and call >= STEPS:
        hole = torch.rand(img, generator=gen) < 1.0 / 3.0
        o[1, NAMES.index(nan_name)] = torch.where(hole, torch.full(img, float("nan"), dtype=dt), o[1, NAMES.index(nan_name)])
    f = f.to(dt)
    return (f[:, 0] if E == 1 else f), o, w


_REF = {}


def restatement(key, clamp=False, cls=None):
    """the fp64 handler (tests/_mhandler_ref.py; ``cls``: a subclass of it) after the PASSES x STEPS updates of a case, computed
    once per process"""
    import _mhandler_ref as mh
    cls = cls or mh.Handler
    if (key, clamp, cls) not in _REF:
        grid, E = key[0], key[1]
        h = cls(NAMES, GRIDS[grid], STEPS, 6, lists(E), ensemble_size=E, climatology=climatology(grid), scale=scale())
        for call in range(PASSES * STEPS):
            prd, tar, w = call_inputs(key, call, clamp)
            h.update(prd, tar, 0.5 + call, call % STEPS, w)
        _REF[(key, clamp, cls)] = h
    return _REF[(key, clamp, cls)]


def _mismatch(a, b):
    import _metrics_ref as ref
    return ref.mismatch(a, b)


# the dedicated clamp case: the observation is the member mean, so L1 and RMSE of the mean are rounding noise and not compared
CLAMP_KEY = (1, 3, f32, False, None)
CLAMP_HANDLES = ("SSR", "Spread", "ACC", "CRPS", "Rank Histogram")


def compare(got_curve, got_counter, want, only=None):
    """every curve and counter of ``got`` ({name: tensor}) against the fp64 handler ``want``: the worst relative L2 over the
    curves and counters, the worst relative error over the occupied histogram bins, whether every empty bin is exactly 0"""
    worst, bins, zeros = 0.0, 0.0, True
    for name, _, _ in want.handles:
        if only is not None and name not in only:
            continue
        c, w = got_curve[name].detach().cpu().double(), want.curve[name]
        assert c.shape == w.shape, (name, c.shape, w.shape)
        if name == "Rank Histogram":
            occ = w > 0
            bins = max(bins, ((c[occ] - w[occ]).abs() / w[occ]).max().item())
            zeros = zeros and bool((c[~occ] == 0).all())
        else:
            worst = max(worst, _mismatch(c, w))
        worst = max(worst, _mismatch(got_counter[name], want.counter[name]))
    return worst, bins, zeros
