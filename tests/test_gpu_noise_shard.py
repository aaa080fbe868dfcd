"""GPU tests of mk_noise_update_shard (csrc/noise.hip) through the C ABI, one process: the update of a BOX of the global state.
The contract under test: element e of one global time level (B, C, R, S) takes normal e & 3 of Philox group e >> 2, wherever it is
stored — so boxes that tile the array, each updated on its own, assemble to exactly what mk_noise_update writes into the whole
array (torch.equal), for groups that straddle a row end (S % 4 = 2), a box edge (s0 % 4 = 2) and for the odd sizes of the grid form.

One case cannot be stated against mk_noise_update: its rows are 2 M floats, so an ODD row length (S = 9) with per-row sigma (the
autoregressive and replace rules) has no serial form.  There the tiles are compared bit for bit with the whole array as ONE box of
the new entry, that one box with the fp64 restatement, and the white draw — which only knows the flat index — with mk_noise_update
on the flattened level."""
import ctypes

import pytest
import torch

import _noise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5          # the bound of test_gpu_noise.py::test_drawn_states_match_the_restatement_from_the_same_seed_and_offset (rel-L2)
WHITE, AR, REPLACE = 0, 1, 2
MODES = {"white": WHITE, "ar": AR, "replace": REPLACE}
B, C, NR = 2, 3, 5
SEED, OFFSET = 2025, 40


def _lib():
    from makani_amd import _lib as L
    return L


def _rng(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _serial(state, xi, sigma, phi, rng, mode, M, reflect):
    """mk_noise_update on the whole (B, T, C, R, 2 M) array, in place"""
    L = _lib()
    Bn, T, Cn, Rn = state.shape[:4]
    L.check(L.lib().mk_noise_update(L.ptr(state), L.ptr(xi), L.ptr(sigma), L.ptr(phi), L.ptr(rng), mode, Bn, T, Cn, Rn, M,
                                    int(reflect), L.stream()), "mk_noise_update")


def _shard(state, xi, sigma, phi, rng, mode, Rg, Sg, r0, s0, reflect):
    """mk_noise_update_shard on the local (B, T, C, Rl, Sl) box at (r0, s0) of the global (R, S) plane, in place"""
    L = _lib()
    Bn, T, Cn, Rl, Sl = state.shape
    L.check(L.lib().mk_noise_update_shard(L.ptr(state), L.ptr(xi), L.ptr(sigma), L.ptr(phi), L.ptr(rng), mode, Bn, T, Cn, Rg, Sg,
                                          r0, Rl, s0, Sl, int(reflect), L.stream()), "mk_noise_update_shard")


def _advance(rng, n):
    L = _lib()
    L.check(L.lib().mk_noise_advance(L.ptr(rng), n, L.stream()), "mk_noise_advance")


def _operands(T, S, seed=0):
    """one non-zero global state and the tables of the update rules"""
    g = torch.Generator().manual_seed(seed)
    state = torch.randn(B, T, C, NR, S, generator=g).to(DEV)
    sigma = (torch.rand(C, NR, generator=g) + 0.5).to(DEV)
    phi = torch.tensor([0.3, 0.6, 0.9], device=DEV)
    return state, sigma, phi


def _boxes(rows, floats):
    r0 = 0
    for Rl in rows:
        s0 = 0
        for Sl in floats:
            yield r0, Rl, s0, Sl
            s0 += Sl
        r0 += Rl


def _tiled(state, sigma, phi, rng, mode, rows, floats, reflect):
    """every box starts from its slice of ``state``, is updated on its own and is put back: the assembled new state"""
    S = state.shape[-1]
    out = torch.full_like(state, float("nan"))
    for r0, Rl, s0, Sl in _boxes(rows, floats):
        box = state[..., r0:r0 + Rl, s0:s0 + Sl].contiguous()
        _shard(box, None, sigma[:, r0:r0 + Rl].contiguous(), phi, rng, mode, NR, S, r0, s0, reflect)
        out[..., r0:r0 + Rl, s0:s0 + Sl] = box
    return out


def _levels(mode, T):
    return 1 if mode == AR else T


# ---- 1. tiling is bit-exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, floats", [(14, [8, 6]), (14, [6, 8]), (10, [5, 5]), (9, [5, 4])],
                         ids=["spectral-s0-8", "spectral-s0-6-split-group", "grid-10", "grid-9-odd"])
@pytest.mark.parametrize("mode", list(MODES))
def test_boxes_that_tile_the_array_assemble_to_the_serial_update_bit_for_bit(S, floats, mode):
    """(B, C, R, S) = (2, 3, 5, S), rows [3, 2] x the given floats; T in {1, 3}, both signs; the autoregressive rule twice with
    the counter advanced in between.  Reference: mk_noise_update on the whole array; for S = 9 see the module docstring."""
    code = MODES[mode]
    for T in (1, 3):
        for reflect in (False, True):
            state, sigma, phi = _operands(T, S)
            rng_t, rng_s = _rng(), _rng()
            want = state.clone()
            got = state
            for _ in range(2 if code == AR else 1):
                got = _tiled(got, sigma, phi, rng_t, code, [3, 2], floats, reflect)
                _advance(rng_t, _levels(code, T))
                if S % 2 == 0:
                    _serial(want, None, sigma, phi, rng_s, code, S // 2, reflect)
                else:
                    _shard(want, None, sigma, phi, rng_s, code, NR, S, 0, 0, reflect)
                _advance(rng_s, _levels(code, T))
            assert not torch.isnan(got).any(), "a box left elements unwritten"
            assert torch.equal(got, want), (mode, T, reflect, S, floats)
            assert rng_t.tolist() == rng_s.tolist() == [SEED, OFFSET + (2 if code == AR else T)]
            if S % 2 and code == WHITE:
                # the white draw knows nothing but the flat index: the level flattened to (1, 1, 1, B C R S / 2, 2)
                flat = torch.zeros(1, T, 1, 1, B * C * NR * S, device=DEV)
                _serial(flat, None, None, None, _rng(), WHITE, B * C * NR * S // 2, reflect)
                assert torch.equal(got, flat.reshape(T, B, C, NR, S).transpose(0, 1))


def test_odd_row_length_as_one_box_matches_the_restatement():
    """the reference of the S = 9 cases above against tests/_noise_ref.py: replace, then one autoregressive step"""
    T, S = 2, 9
    state, sigma, phi = _operands(T, S)
    rng = _rng()
    sg, ph = sigma.double().cpu().numpy(), phi.double().cpu().numpy()
    inner = (C, NR, S, 1)                       # the restatement's (C, L, M, 2) with the row as M and a pair of one
    _shard(state, None, sigma, phi, rng, REPLACE, NR, S, 0, 0, False)
    want = R.update(None, R.draw(SEED, OFFSET, T, B, inner), "replace", sg, ph)
    assert R.rel_l2(state.cpu().numpy(), want[..., 0]) <= TOL
    _advance(rng, T)
    _shard(state, None, sigma, phi, rng, AR, NR, S, 0, 0, False)
    want = R.update(want, R.draw(SEED, OFFSET + T, 1, B, inner), "ar", sg, ph)
    assert R.rel_l2(state.cpu().numpy(), want[..., 0]) <= TOL


# ---- 2. the whole array as one box -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn, Rn, M, misalign", [(3, 5, 7, 0), (2, 8, 8, 0), (3, 5, 7, 1), (2, 33, 33, 0)],
                         ids=["8-byte", "16-byte", "4-byte-pointer", "several-blocks"])
def test_the_whole_array_as_one_box_equals_mk_noise_update(Cn, Rn, M, misalign):
    S = 2 * M
    g = torch.Generator().manual_seed(1)
    sigma = (torch.rand(Cn, Rn, generator=g) + 0.5).to(DEV)
    phi = torch.linspace(0.2, 0.9, Cn).to(DEV)
    for mode in (WHITE, AR, REPLACE):
        for T in (1, 2):
            n = B * T * Cn * Rn * S
            start = torch.randn(n, generator=g).to(DEV)
            bufs = [torch.zeros(n + 4, device=DEV) for _ in range(2)]
            a, b = (buf[misalign:misalign + n].view(B, T, Cn, Rn, S) for buf in bufs)
            a.copy_(start.view_as(a))
            b.copy_(start.view_as(b))
            _serial(a, None, sigma, phi, _rng(), mode, M, True)
            _shard(b, None, sigma, phi, _rng(), mode, Rn, S, 0, 0, True)
            assert torch.equal(a, b), (mode, T)
            assert not torch.equal(a, start.view_as(a))
            assert all(not buf[:misalign].any() and not buf[misalign + n:].any() for buf in bufs), "wrote outside the state"


# ---- 3. against the restatement ------------------------------------------------------------------------------------------------
def test_the_assembled_state_matches_the_restatement_on_the_global_shape():
    T, S = 2, 14
    state, sigma, phi = _operands(T, S)
    rng = _rng()
    sg, ph = sigma.double().cpu().numpy(), phi.double().cpu().numpy()
    inner = (C, NR, S // 2, 2)
    got = _tiled(state, sigma, phi, rng, REPLACE, [3, 2], [6, 8], False)
    want = R.update(None, R.draw(SEED, OFFSET, T, B, inner), "replace", sg, ph)
    err = R.rel_l2(got.cpu().numpy().reshape(want.shape), want)
    print(f"replace, tiled: rel-L2 {err:.2e}")
    assert err <= TOL
    _advance(rng, T)
    got = _tiled(got, sigma, phi, rng, AR, [3, 2], [6, 8], False)
    want = R.update(want, R.draw(SEED, OFFSET + T, 1, B, inner), "ar", sg, ph)
    err = R.rel_l2(got.cpu().numpy().reshape(want.shape), want)
    print(f"autoregressive step, tiled: rel-L2 {err:.2e}")
    assert err <= TOL
    white = _tiled(state, sigma, phi, _rng(7, 3), WHITE, [3, 2], [6, 8], True)
    want = R.update(None, R.draw(7, 3, T, B, inner), "white", reflect=True)
    assert R.rel_l2(white.cpu().numpy().reshape(want.shape), want) <= TOL


# ---- 4. given innovations ------------------------------------------------------------------------------------------------------
def test_given_innovations_are_applied_box_locally_and_leave_the_counter_alone():
    """the box's own (sigma rows, xi) decide, not its place in the global array.  Bound: the kernel rounds phi v, sigma xi and
    their sum (fused or not) — at most 4 roundings of 2^-24 relative to |phi v| + |sigma xi|."""
    T, S, r0, Rl, s0, Sl = 2, 14, 3, 2, 6, 8
    state, sigma, phi = _operands(T, S)
    g = torch.Generator().manual_seed(5)
    box = state[..., r0:r0 + Rl, s0:s0 + Sl].contiguous()
    old = box.clone()
    sg = sigma[:, r0:r0 + Rl].contiguous()
    rng = _rng()
    xi = torch.randn(B, 1, C, Rl, Sl, generator=g).to(DEV)
    _shard(box, xi, sg, phi, rng, AR, NR, S, r0, s0, False)
    a, b = phi.view(1, C, 1, 1) * old[:, 1], sg.view(1, C, Rl, 1) * xi[:, 0]
    assert torch.equal(box[:, 0], old[:, 1])
    assert bool(((box[:, 1] - (a + b)).abs() <= 4 * 2.0 ** -24 * (a.abs() + b.abs())).all())
    xi = torch.randn(B, T, C, Rl, Sl, generator=g).to(DEV)
    _shard(box, xi, None, None, rng, WHITE, NR, S, r0, s0, True)
    assert torch.equal(box, -xi)
    assert rng.tolist() == [SEED, OFFSET]


# ---- 5. bad arguments ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_a_negative_status_and_leave_the_state_alone():
    L = _lib()
    lib = L.lib()
    T, S = 1, 14
    state, sigma, phi = _operands(T, S)
    keep = state.clone()
    rng = _rng()
    null = ctypes.c_void_p(0)

    def call(st=None, xi=null, sg=None, ph=None, rg=None, mode=AR, dims=(B, T, C, NR, S), box=(0, NR, 0, S)):
        p = [L.ptr(state) if st is None else st, xi, L.ptr(sigma) if sg is None else sg, L.ptr(phi) if ph is None else ph,
             L.ptr(rng) if rg is None else rg]
        return lib.mk_noise_update_shard(*p, mode, *dims, *box, 0, L.stream())

    for kw, msg in ((dict(st=null), b"null state"), (dict(rg=null), b"null rng"), (dict(sg=null), b"null sigma"),
                    (dict(ph=null), b"null sigma"), (dict(mode=3), b"unknown mode 3"), (dict(dims=(B, 0, C, NR, S)), b"T >= 1"),
                    (dict(dims=(B, T, C, 0, S)), b"bad shape"), (dict(box=(3, 3, 0, S)), b"rows [3, 3 + 3) leave"),
                    (dict(box=(-1, 2, 0, S)), b"rows"), (dict(box=(0, 0, 0, S)), b"rows"),
                    (dict(box=(0, NR, 8, 8)), b"floats [8, 8 + 8) leave"), (dict(box=(0, NR, -2, 4)), b"floats"),
                    (dict(box=(0, NR, 0, 0)), b"floats"), (dict(dims=(B, T, 1 << 15, 1 << 8, 1 << 9)), b"2^31")):
        assert call(**kw) < 0 and msg in lib.mk_last_error(), (kw, lib.mk_last_error())
    torch.cuda.synchronize()
    assert torch.equal(state, keep) and rng.tolist() == [SEED, OFFSET]
