"""``LossHandler`` across ranks, in the pattern of tests/test_gpu_preproc_dist.py: the processes share cuda:0 over gloo, under one
time limit each.

* h2 x w2 (four processes), grid 17 x 32 (latitudes split [9, 8]): the mixed list of the recorded cases — l2 with "auto" weights and
  the time-difference scale, the ensemble CRPS of the tendency, the drift regularization and the moist hydrostatic loss — on this
  rank's shard against the serial handler on the whole sphere;
* an "ensemble" group of two (two processes), E = 4: every rank holds two members; l2 of the ensemble mean, CRPS and drift against
  the serial handler with all four.

The scalar is the same on every rank and within 1e-5 of the serial one; the gradient of this rank's shard / members is within
1e-5 (rel-L2) of the slice of the serial gradient.  RCCL with more than one GPU is not exercised here."""
import pytest
import torch

from _ranks import launch, ranks, rel

pytestmark = pytest.mark.gpu
IMG, B, NH = (17, 32), 2, 1
NAMES = "u10m t2m z500 z850 z1000 t500 t850 t1000 q500 q850 q1000".split()
C = len(NAMES)
L2 = {"type": "l2", "channel_weights": "auto", "temp_diff_normalization": True}
CRPS = {"type": "ensemble_crps", "relative_weight": 0.5}
DRIFT = {"type": "drift_regularization", "parameters": {"p": 2}}
HYDRO = {"type": "hydrostatic", "parameters": {"p_min": 400, "use_moist_air_formula": True}, "relative_weight": 1e-4}


def _stats():
    import math
    bias, scale = [], []
    for n in NAMES:
        if n in ("u10m", "t2m"):
            b, s = {"u10m": (0.5, 5.0), "t2m": (278.0, 21.0)}[n]
        else:
            k = math.log(1000.0 / int(n[1:])) / math.log(20.0)
            b, s = {"z": (600.0 + 6.9e4 * k, 3.0e3 * (0.8 + 0.4 * k)), "t": (285.0 - 70.0 * k, 15.0 - 6.0 * k),
                    "q": (2.0e-3 * (1.0 - k) ** 3 + 2e-6, 2.0e-3 * (1.0 - k) ** 3 + 1e-6)}[n[0]]
        bias.append(b)
        scale.append(s)
    bias, scale = torch.tensor(bias).view(1, C, 1, 1), torch.tensor(scale).view(1, C, 1, 1)
    return bias, scale, scale.reshape(-1) * torch.linspace(0.2, 0.7, C)


def _tensors(E):
    g = torch.Generator().manual_seed(23)
    return dict(prd=torch.randn(B, E, C, *IMG, generator=g), tar=torch.randn(B, C, *IMG, generator=g),
                inp=torch.randn(B, (NH + 1) * C, *IMG, generator=g))


def _run(ma, losses, t, cut, members, dev):
    """scalar and gradient of a handler built under the process groups as they are now, on the cut tensors"""
    from _losshandler_ref import Params
    bias, scale, tds = _stats()
    params = Params(n_future=0, n_history=NH, img_shape_x_resampled=IMG[0], img_shape_y_resampled=IMG[1], img_crop_offset_x=0,
                    img_crop_offset_y=0, channel_names=NAMES, out_channels=list(range(C)), model_grid_type="equiangular", losses=losses)
    h = ma.LossHandler(params, bias=bias, scale=scale, time_diff_stds=tds).to(dev).train()
    prd = t["prd"][:, members][cut].contiguous().to(dev).requires_grad_(True)
    loss = h(prd, t["tar"][cut].contiguous().to(dev), None, t["inp"][cut].contiguous().to(dev))
    (grad,) = torch.autograd.grad(loss, prd)
    return h, loss.detach(), grad


def _same_on_every_rank(dist, world, loss):
    mine = loss.cpu().reshape(1)
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    assert all(torch.equal(e, every[0]) for e in every), "the scalar differs between ranks"


def _worker_spatial(rank, world, rendezvous):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        dev = torch.device("cuda:0")
        losses = [L2, dict(CRPS, tendency=True), DRIFT, HYDRO]
        t = _tensors(2)
        full = (Ellipsis, slice(None), slice(None))
        hs, want, gwant = _run(ma, losses, t, full, slice(None), dev)
        assert not hs.spatial_distributed
        _, ih, iw = mcomm.init(2, 2)
        assert thd.ensure_initialized()
        lat, lon = thd.compute_split_shapes(IMG[0], 2), thd.compute_split_shapes(IMG[1], 2)
        assert lat == [9, 8] and lon == [16, 16]
        cut = (Ellipsis, slice(sum(lat[:ih]), sum(lat[:ih + 1])), slice(sum(lon[:iw]), sum(lon[:iw + 1])))
        hd, got, ggot = _run(ma, losses, t, cut, slice(None), dev)
        assert hd.spatial_distributed and all(getattr(f, "spatial_distributed") for f in hd.loss_fn)
        _same_on_every_rank(dist, world, got)
        errs = dict(loss=rel(got, want), grad=rel(ggot, gwant[cut]))
        print(f"h2w2 rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
        assert max(errs.values()) <= 1e-5, (rank, errs)


def _worker_ensemble(rank, world, rendezvous):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        dev = torch.device("cuda:0")
        losses = [L2, CRPS, DRIFT]
        t = _tensors(4)
        full = (Ellipsis, slice(None), slice(None))
        hs, want, gwant = _run(ma, losses, t, full, slice(None), dev)
        assert not hs.ensemble_distributed
        mcomm.init(1, 1, ensemble=2)
        me = mcomm.get_rank("ensemble")
        members = slice(2 * me, 2 * me + 2)
        hd, got, ggot = _run(ma, losses, t, full, members, dev)
        assert hd.ensemble_distributed and mcomm.get_size("ensemble") == 2
        _same_on_every_rank(dist, world, got)
        errs = dict(loss=rel(got, want), grad=rel(ggot, gwant[:, members]))
        print(f"ensemble rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
        assert max(errs.values()) <= 1e-5, (rank, errs)


def test_h2_w2_shards_equal_the_serial_handler():
    launch(_worker_spatial, 4, limit=240)


def test_ensemble_group_of_two_equals_the_serial_handler():
    launch(_worker_ensemble, 2, limit=240)
