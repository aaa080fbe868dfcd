"""``MetricsHandler`` across ranks, in the pattern of tests/test_gpu_losshandler_dist.py: the processes share cuda:0 over gloo, each
test under its own time limit, and the first failing rank ends the others.  Grid 17 x 32, the lists and inputs of
tests/_mrollout_cases.py, three ``idt`` rows.

* h2 x w2 (four processes; latitudes split [9, 8]): the fused handler on this rank's shard — the climatology is cut by the
  constructor, the ``(B, J, K)`` sums are all-reduced once per update — against the serial handler on the whole sphere: <= 1e-5
  per curve and counter, and bit-identical on every rank.
* a "batch" group of two: every rank feeds one half of the samples, then ``reduce()`` + ``finalize()``, against the serial
  handler fed both halves.
* an "ensemble" group of two, E = 4: every rank holds two members and takes the composed path, against the serial handler with
  all four.
RCCL with more than one GPU is not exercised here."""
import pytest
import torch

from _ranks import launch, ranks

pytestmark = pytest.mark.gpu
TOL = 1e-5
GRID = 1          # 17 x 32


def _handler(ma, E, dev):
    import _mrollout_cases as cases
    from _losshandler_ref import Params
    img = cases.GRIDS[GRID]
    params = Params(channel_names=cases.NAMES, dt=1, dhours=6, img_shape_x_resampled=img[0], img_shape_y_resampled=img[1], ensemble_size=E)
    h = ma.MetricsHandler(params, cases.climatology(GRID), cases.STEPS, dev, scale=cases.scale(), **cases.lists(E))
    h.initialize_buffers()
    h.zero_buffers()
    return h


def _feed(h, key, dev, cut=(Ellipsis,), members=slice(None), samples=slice(None)):
    import _mrollout_cases as cases
    for call in range(cases.STEPS):
        prd, tar, w = cases.call_inputs(key, call)
        h.update(prd[samples][:, members][cut].contiguous().to(dev), tar[samples][cut].contiguous().to(dev),
                 torch.tensor(0.5 + call, device=dev), call, w[samples][cut].contiguous().to(dev) if w is not None else None)


def _errors(h, serial, finalized=False):
    import _mrollout_cases as cases
    errs = {}
    for m, s in zip(h.metric_handles, serial.metric_handles):
        a, b = (m.rollout_curve_cpu, s.rollout_curve_cpu) if finalized else (m.rollout_curve, s.rollout_curve)
        assert bool(torch.isfinite(b).all()) and float(b.abs().sum()) > 0, m.metric_name
        if m.metric_name == "Rank Histogram":
            a, b = a.double().cpu(), b.double().cpu()
            occ = b > 0
            errs[m.metric_name] = float(((a[occ] - b[occ]).abs() / b[occ]).max())
            assert bool((a[~occ] == 0).all())
        else:
            errs[m.metric_name] = cases._mismatch(a, b)
        if not finalized:
            errs[m.metric_name + " n"] = cases._mismatch(m.rollout_counter, s.rollout_counter)
    return errs


def _same_on_every_rank(dist, world, t):
    mine = t.detach().cpu().contiguous()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    assert all(torch.equal(e, every[0]) for e in every), "the buffers differ between ranks"


def _worker_spatial(rank, world, rendezvous):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        import _mrollout_cases as cases
        dev = torch.device("cuda:0")
        key = (GRID, 3, cases.f32, True, None)
        serial = _handler(ma, 3, dev)
        assert not serial.spatial_distributed
        _feed(serial, key, dev)
        _, ih, iw = mcomm.init(2, 2)
        assert thd.ensure_initialized()
        img = cases.GRIDS[GRID]
        lat, lon = thd.compute_split_shapes(img[0], 2), thd.compute_split_shapes(img[1], 2)
        assert lat == [9, 8] and lon == [16, 16]
        cut = (Ellipsis, slice(sum(lat[:ih]), sum(lat[:ih + 1])), slice(sum(lon[:iw]), sum(lon[:iw + 1])))
        h = _handler(ma, 3, dev)
        assert h.spatial_distributed and h._shared_quadrature and h._clim.shape == (3, lat[ih] * lon[iw])
        assert h._fused(torch.empty(0, device=dev), 3)
        _feed(h, key, dev, cut=cut)
        errs = _errors(h, serial)
        print(f"h2w2 rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
        assert max(errs.values()) <= TOL, (rank, errs)
        _same_on_every_rank(dist, world, h._flat)
        gathered = h._gather_input(cases.call_inputs(key, 0)[1][cut].contiguous().to(dev))
        assert torch.equal(gathered.cpu(), cases.call_inputs(key, 0)[1])


def _worker_batch(rank, world, rendezvous):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import _mrollout_cases as cases
        dev = torch.device("cuda:0")
        key = (GRID, 3, cases.f32, False, None)
        serial = _handler(ma, 3, dev)
        for half in (slice(0, 1), slice(1, 2)):
            _feed(serial, key, dev, samples=half)
        want = serial.finalize()
        mcomm.init(1, 1)
        assert mcomm.get_size("batch") == 2 and mcomm.get_rank("batch") == rank
        h = _handler(ma, 3, dev)
        _feed(h, key, dev, samples=slice(rank, rank + 1))
        logs = h.finalize()
        errs = _errors(h, serial, finalized=True)
        errs["integral"] = cases._mismatch(h._by_name["ACC"].rollout_integral_cpu, serial._by_name["ACC"].rollout_integral_cpu)
        print(f"batch rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
        assert max(errs.values()) <= TOL, (rank, errs)
        assert logs["base"] == want["base"] and list(logs["metrics"]) == list(want["metrics"])
        assert bool((h._by_name["L1"].rollout_counter == 2.0).all())
        _same_on_every_rank(dist, world, h._flat)


def _worker_ensemble(rank, world, rendezvous):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import _mrollout_cases as cases
        dev = torch.device("cuda:0")
        key = (GRID, 4, cases.f32, True, None)
        serial = _handler(ma, 4, dev)
        assert not serial.ensemble_distributed
        _feed(serial, key, dev)
        mcomm.init(1, 1, ensemble=2)
        me = mcomm.get_rank("ensemble")
        assert mcomm.get_size("ensemble") == 2
        h = _handler(ma, 4, dev)
        assert h.ensemble_distributed and not h._fused(torch.empty(0, device=dev), 2)
        _feed(h, key, dev, members=slice(2 * me, 2 * me + 2))
        errs = _errors(h, serial)
        print(f"ensemble rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
        assert max(errs.values()) <= TOL, (rank, errs)


def test_h2_w2_shards_equal_the_serial_handler():
    launch(_worker_spatial, 4, limit=240)


def test_a_batch_group_of_two_reduces_to_the_serial_handler():
    launch(_worker_batch, 2, limit=240)


def test_an_ensemble_group_of_two_takes_the_composed_path_and_equals_serial():
    launch(_worker_ensemble, 2, limit=240)
