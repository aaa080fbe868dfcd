"""``Preprocessor2D`` on a sphere split over h x w ranks: four processes (h2 w2) sharing cuda:0 over gloo, in the pattern of
tests/test_gpu_noise_dist.py, under one time limit.  Grid 19 x 36: the latitudes split [10, 9] (uneven), the longitudes [18, 18].

Every rank holds its shard of the window, the unpredicted features, the noise, the static planes and the bias field.  The
statistics of every rank equal each other bit for bit (merged in rank order from the gathered fp64 triples) and are within 1e-6 of
the serial ones; output shards and window- / noise-gradient shards are within 1e-5 of the slices of the serial result.  The loss
sum(out r1) + sum(finish(yn) r2) sends a gradient to the statistics on every rank, so backward all-reduces the partials of G.
RCCL with more than one GPU is not exercised here."""
import pytest
import torch

from _ranks import launch, ranks, rel

pytestmark = pytest.mark.gpu
IMG, B, C, U, N, S, NH = (19, 36), 2, 3, 2, 1, 2, 1
T = NH + 1


class _ParamNoise(torch.nn.Module):
    def __init__(self, field):
        super().__init__()
        self.state = torch.nn.Parameter(field.clone())

    def forward(self):
        return self.state

    def update(self, replace_state=False, batch_size=None):
        pass

    def is_stateful(self):
        return False


def _tensors():
    g = torch.Generator().manual_seed(17)

    def field(*shape, mean=0.0):
        return torch.randn(shape, generator=g) * 1.5 + mean

    return dict(win=field(B, T * C, *IMG, mean=3.0), unp=field(B, T, U, *IMG, mean=-2.0), noi=field(B, T, N, *IMG),
                static=field(1, S, *IMG), bias=0.2 * field(1, C, *IMG), yn=field(B, C, *IMG), r1=field(B, T * (C + U + N) + S, *IMG),
                r2=field(B, C, *IMG))


def _run(ma, t, cut, dev, distributed):
    """forward and backward on the tensors cut to ``cut``: the output, the statistics, y, and the gradients of window and noise"""
    x = {k: v[cut].contiguous().to(dev) for k, v in t.items()}
    pre = ma.Preprocessor2D(img_shape=IMG, n_history=NH, history_normalization_mode="mean", static_features=x["static"],
                            bias_correction=x["bias"], input_noise=ma.InputNoise(_ParamNoise(x["noi"]), n_history=NH),
                            spatial_distributed=distributed).to(dev)
    pre.train()
    assert pre.spatial_distributed == distributed
    pre.cache_unpredicted_features(None, None, x["unp"], None)
    win = x["win"].requires_grad_(True)
    out = pre.assemble(win)
    y = pre.finish(x["yn"])
    gwin, gnoi = torch.autograd.grad((out * x["r1"]).sum() + (y * x["r2"]).sum(), [win, pre.noise_stage.input_noise.state])
    return dict(out=out.detach(), mean=pre.history_mean.detach(), std=pre.history_std.detach(), y=y.detach(), gwin=gwin, gnoi=gnoi)


def _worker(rank, world, rendezvous):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        dev = torch.device("cuda:0")
        t = _tensors()
        full = (Ellipsis, slice(None), slice(None))
        want = _run(ma, t, full, dev, False)
        _, ih, iw = mcomm.init(2, 2)
        assert thd.ensure_initialized()
        lat, lon = thd.compute_split_shapes(IMG[0], 2), thd.compute_split_shapes(IMG[1], 2)
        assert lat == [10, 9] and lon == [18, 18]
        cut = (Ellipsis, slice(sum(lat[:ih]), sum(lat[:ih + 1])), slice(sum(lon[:iw]), sum(lon[:iw + 1])))
        got = _run(ma, t, cut, dev, True)
        assert tuple(got["out"].shape) == (B, T * (C + U + N) + S, lat[ih], lon[iw])
        # the statistics: the same bits on every rank, the serial values within 1e-6
        mine = torch.stack([got["mean"], got["std"]]).cpu()
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, every[0]) for e in every), "the statistics differ between ranks"
        errs = dict(mean=rel(got["mean"], want["mean"]), std=rel(got["std"], want["std"]))
        assert max(errs.values()) <= 1e-6, (rank, errs)
        for k in ("out", "y", "gwin", "gnoi"):
            errs[k] = rel(got[k], want[k][cut])
            assert errs[k] <= 1e-5, (rank, k, errs[k])
        print(f"h2w2 rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)


def test_h2_w2_shards_equal_the_serial_preprocessor():
    launch(_worker, 4, limit=240)
