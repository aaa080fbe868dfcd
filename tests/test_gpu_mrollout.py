"""The fused ``MetricsHandler.update`` (csrc/mrollout.hip, makani_amd/metric.py) on the GPU against the fp64 restatement of
tests/_mhandler_ref.py: <= 1e-5 relative L2 per curve and counter, occupied histogram bins per entry <= 1e-5, empty bins exactly 0
(the project's metric gate: tests/test_gpu_metrics.py).  The cases and the conditioning of their inputs are those of
tests/_mrollout_cases.py; tests/test_metricshandler.py asserts on the CPU that the reference formula in plain fp32 torch meets
the same gate on them.

Every case: three ``idt`` rows over two passes (the merge runs, RMSE's root of the sum of squares included), C = 11 with lists
that are out of order and non-contiguous, grids 9 x 14 (one point per thread and a tail), 17 x 32 (one chunk, 16-byte path) and
91 x 180 (16 chunks, a partial last block), E in {1, 2, 3, 9, 32}, f32 and bf16 (the restatement scores the rounded values), with
and without weight, NaN targets on the second pass in a channel of one list or of every list."""
import pytest
import torch

import _mrollout_cases as cases
from _losshandler_ref import Params

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"


def _handler(key, **kw):
    import makani_amd as ma
    grid, E = key[0], key[1]
    img = cases.GRIDS[grid]
    params = Params(channel_names=cases.NAMES, dt=1, dhours=6, img_shape_x_resampled=img[0], img_shape_y_resampled=img[1], ensemble_size=E)
    h = ma.MetricsHandler(params, cases.climatology(grid), cases.STEPS, torch.device(DEV), scale=cases.scale(), **cases.lists(E), **kw)
    h.initialize_buffers()
    h.zero_buffers()
    return h


def _feed(h, key, clamp=False):
    for call in range(cases.PASSES * cases.STEPS):
        prd, tar, w = cases.call_inputs(key, call, clamp)
        h.update(prd.to(DEV), tar.to(DEV), torch.tensor(0.5 + call, device=DEV), call % cases.STEPS, w.to(DEV) if w is not None else None)
    return h


def _buffers(h):
    return {m.metric_name: m.rollout_curve for m in h.metric_handles}, {m.metric_name: m.rollout_counter for m in h.metric_handles}


def _check(h, want, what, only=None):
    worst, bins, zeros = cases.compare(*_buffers(h), want, only)
    print(f"{what}: curves and counters {worst:.2e}, occupied bins {bins:.2e}, empty bins exactly 0: {zeros}")
    assert worst <= TOL and bins <= TOL and zeros, (what, worst, bins, zeros)


@pytest.mark.parametrize("key", cases.CASES, ids=cases.case_id)
def test_the_fused_update_matches_the_restatement(key):
    want = cases.restatement(key)
    h = _feed(_handler(key), key)
    _check(h, want, cases.case_id(key))
    # counts: the quadrature weight under NaN targets or weights (compared above), exactly the number of samples otherwise
    exact = float(cases.B * cases.PASSES)
    for m in h.metric_handles:
        if not key[3] and (key[4] is None or key[4] not in m.metric_channels):
            assert bool((m.rollout_counter == exact).all()), m.metric_name
        elif not key[3]:
            i = m.metric_channels.index(key[4])
            assert float(m.rollout_counter[0, i].reshape(-1)[0]) < exact - 0.1
    # finalize() and report() against the restatement
    final, integral, wlogs = want.finalize()
    logs = h.finalize()
    for m in h.metric_handles:
        if m.metric_name == "Rank Histogram":
            occ = final[m.metric_name] > 0
            got = m.rollout_curve_cpu.double()
            assert float(((got[occ] - final[m.metric_name][occ]).abs() / final[m.metric_name][occ]).max()) <= TOL
        else:
            assert cases._mismatch(m.rollout_curve_cpu, final[m.metric_name]) <= TOL, m.metric_name
    assert cases._mismatch(h._by_name["ACC"].rollout_integral_cpu, integral["ACC"]) <= TOL
    assert [k for k in logs["metrics"] if k != "rollouts"] == list(wlogs["metrics"])
    assert logs["base"]["validation steps"] == wlogs["base"]["validation steps"] == cases.PASSES
    assert abs(logs["base"]["validation loss"] - wlogs["base"]["validation loss"]) <= 1e-6 * abs(wlogs["base"]["validation loss"])
    for m in h.metric_handles:          # the log entries are entries of the finalized curves, which were compared above
        if m.report_metric:
            for i, var in enumerate(m.metric_channels):
                got = logs["metrics"][f"validation {m.metric_name} {var}({cases.STEPS * 6})"]
                assert got == m.rollout_curve_cpu[cases.STEPS - 1, i].item() or got != got, (m.metric_name, var)
    log, table = h._by_name["RMSE"].report(index=1, table=True)
    assert list(log) == [f"RMSE {c}(12)" for c in h.rmse_var_names] and len(table) == cases.STEPS * len(h.rmse_var_names)
    assert table[0][:3] == ["RMSE", h.rmse_var_names[0], 6]


def test_the_clamp_of_ssr_is_active_when_the_observation_is_the_member_mean():
    key = cases.CLAMP_KEY
    want = cases.restatement(key, clamp=True)
    h = _feed(_handler(key), key, clamp=True)
    _check(h, want, "clamp", cases.CLAMP_HANDLES)
    spread = h._by_name["Spread"]          # the clamped value is sqrt(spread^2 / eps): three orders above an unclamped ratio
    assert float(h.ssr_curve.min()) > 100.0 and torch.isfinite(h.ssr_curve).all() and torch.isfinite(spread.rollout_curve).all()


@pytest.mark.parametrize("key", [cases.CASES[1], cases.CASES[4], cases.CASES[9], cases.CASES[8]], ids=cases.case_id)
def test_the_fused_and_the_composed_path_agree(key):
    want = cases.restatement(key)
    fused, composed = _feed(_handler(key), key), _handler(key)
    composed.use_fused = False
    _feed(composed, key)
    _check(composed, want, "composed " + cases.case_id(key))
    fc, fn = _buffers(fused)
    for m in composed.metric_handles:
        a, b = m.rollout_curve, fc[m.metric_name]
        if m.metric_name == "Rank Histogram":
            occ = a > 0
            assert float(((a[occ] - b[occ]).abs() / a[occ]).max()) <= TOL and bool((b[~occ] == 0).all())
        else:
            assert cases._mismatch(b, a) <= TOL, m.metric_name
        assert cases._mismatch(fn[m.metric_name], m.rollout_counter) <= TOL, m.metric_name
    assert torch.equal(fused.valid_buffer, composed.valid_buffer)


def test_two_fused_runs_are_bit_identical():
    key = cases.CASES[9]
    a, b = _feed(_handler(key), key), _feed(_handler(key), key)
    assert torch.equal(a._flat, b._flat) and float(a._flat.abs().sum()) > 0
    # the sums themselves: two launches on the same inputs
    import makani_amd.metric as mm
    from makani_amd._lib import check, dtype_code, lib, ptr, stream
    prd, tar, w = (t.to(DEV) for t in cases.call_inputs(key, 4))
    Bn, E, C, H, W = prd.shape
    K, J, ch = mm._NSUM + E + 1, a._J, lib().mk_metric_chunks(H * W)
    outs = []
    for _ in range(2):
        part = torch.empty(Bn * J * ch * K, device=DEV)
        sums = torch.empty(Bn, J, K, device=DEV)
        check(lib().mk_mrollout_sums(ptr(prd), dtype_code(prd), ptr(tar), dtype_code(tar), ptr(w), ptr(a._quad), ptr(a._clim), ptr(a._table),
                                     ptr(part), ptr(sums), Bn, E, C, J, a._clim.shape[0], H * W, 1, stream()), "mk_mrollout_sums")
        outs.append((part, sums))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][1][..., 1].sum()) > 0          # the NaN points of the second pass are counted


def test_an_update_replays_from_a_captured_graph():
    """``update(..., idt=0)`` captured once, replayed three times on refreshed static inputs (the second holds NaN targets, so
    ``counts_new`` changes its form on the device), equals three eager updates bit for bit"""
    key = (1, 3, cases.f32, False, "z500")
    inputs = [cases.call_inputs(key, call)[:2] for call in (0, 3, 1)]          # call 3: the second pass, with NaN
    assert bool(torch.isnan(inputs[1][1]).any()) and not bool(torch.isnan(inputs[0][1]).any())
    eager = _handler(key)
    loss = torch.tensor(0.75, device=DEV)
    for prd, tar in inputs:
        eager.update(prd.to(DEV), tar.to(DEV), loss, 0)
    h = _handler(key)
    sp, st = inputs[0][0].to(DEV).clone(), inputs[0][1].to(DEV).clone()
    h.update(sp, st, loss, 0)                                # loads the library outside the capture
    h.zero_buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            h.update(sp, st, loss, 0)
    torch.cuda.current_stream().wait_stream(s)
    h.zero_buffers()
    for prd, tar in inputs:
        sp.copy_(prd)
        st.copy_(tar)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(h._flat, eager._flat) and torch.equal(h.valid_buffer, eager.valid_buffer)
    z = h._by_name["L1"].metric_channels.index("z500")          # two replays counted samples, the one with NaN quadrature weight
    assert float(h.valid_steps) == 3.0 and 4.0 < float(h._by_name["L1"].rollout_counter[0, z]) < 6.0 - 0.1
