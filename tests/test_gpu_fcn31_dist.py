"""FourCastNet3.1 under h x w spatial model parallelism, validated on ONE GPU: several processes share cuda:0 and exchange through
gloo, each holds its latitude / longitude shard of the input (NaN sea-surface temperature and land mask included), and the results
are compared with the serial HIP network on the shard, with the gates of tests/test_gpu_fcn3_distributed.py: output 1e-4, input
gradient 2e-4, parameter gradients 5e-4 or within 1e-4 of the largest gradient magnitude.  The ``global_conv.weight`` gradient is
sliced over l and reduced over w; the position-embedding gradient is compared on its latitude shard after the reduction over w."""
import json
import os

import pytest
import torch

from _ranks import hw_groups, launch, ranks, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shard(t, lat_shapes, lon_shapes, ih, iw):
    a, b = sum(lat_shapes[:ih]), sum(lon_shapes[:iw])
    return t[..., a:a + lat_shapes[ih], b:b + lon_shapes[iw]]


def _worker(rank, world, rendezvous, h, w, name):
    with ranks(rank, world, rendezvous) as dist:
        ih, iw, hg, wg = hw_groups(rank, h, w)
        import numpy as np
        import makani_amd as ma
        import makani_amd.distributed as thd
        dev = torch.device("cuda:0")
        g = np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False)
        kwargs = json.loads(str(g["kwargs"]))
        sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
        serial = ma.AtmoSphericNeuralOperatorNet31(**kwargs)          # (thd not initialised yet: the serial operators)
        serial.load_state_dict(sd, strict=True)
        serial = serial.to(dev)
        x = torch.from_numpy(g["x"]).to(dev)
        G = torch.from_numpy(g["g"]).to(dev)
        xs = x.clone().requires_grad_(True)
        ys = serial(xs)
        (ys * G).sum().backward()

        thd.init(hg if h > 1 else None, wg if w > 1 else None, dist.group.WORLD)
        model = ma.AtmoSphericNeuralOperatorNet31(**kwargs).to(dev)
        assert isinstance(model.sht, thd.DistributedRealSHT)
        lat = thd.compute_split_shapes(kwargs["inp_shape"][0], h)
        lon = thd.compute_split_shapes(kwargs["inp_shape"][1], w)
        lat_in = thd.compute_split_shapes(model.h, h)          # the internal grid: the position embedding's latitudes
        p0, pl = sum(lat_in[:ih]), lat_in[ih]
        l0, ll = sum(model.isht.l_shapes[:ih]), model.isht.l_shapes[ih]
        own = model.state_dict()
        for k in own:
            src = sd[k].to(dev)
            if k.endswith("global_conv.weight"):
                src = src[..., l0:l0 + ll]
            if k == "pos_embed.position_embeddings":
                src = src[:, :, p0:p0 + pl]
            assert own[k].shape == src.shape, (k, own[k].shape, src.shape)
            own[k].copy_(src)
        xl = _shard(x, lat, lon, ih, iw).clone().requires_grad_(True)
        yl = model(xl)
        (yl * _shard(G, lat, lon, ih, iw)).sum().backward()
        e_y = rel(yl, _shard(ys, lat, lon, ih, iw))
        e_gx = rel(xl.grad, _shard(xs.grad, lat, lon, ih, iw))
        assert torch.isfinite(yl).all() and torch.isfinite(xl.grad).all()
        assert e_y < 1e-4 and e_gx < 2e-4, (rank, e_y, e_gx)
        sref = dict(serial.named_parameters())
        gmax = max(float(p.grad.abs().max()) for p in sref.values())
        for k, p in model.named_parameters():
            gp = (torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).detach().cpu().contiguous()
            if k.endswith("global_conv.weight"):                     # sharded over h, shared over w
                if w > 1:
                    dist.all_reduce(gp, group=wg)
                ref = sref[k].grad[..., l0:l0 + ll].contiguous()
                ref = (torch.view_as_real(ref) if ref.is_complex() else ref).cpu()
            elif k == "pos_embed.position_embeddings":               # sharded over h, shared over w
                if w > 1:
                    dist.all_reduce(gp, group=wg)
                ref = sref[k].grad[:, :, p0:p0 + pl].cpu()
            else:
                dist.all_reduce(gp)
                ref = sref[k].grad.cpu()
            e, a = rel(gp, ref), (gp - ref).abs().max().item()
            assert e < 5e-4 or a < 1e-4 * gmax, (rank, k, e, a)


@pytest.mark.parametrize("h,w,name", [(2, 1, "fcn31_small_33x64.npz"), (1, 2, "fcn31_small_33x64.npz"),
                                      (2, 2, "fcn31_small_33x64.npz"), (2, 2, "fcn31_history_24x48.npz")])
def test_spatial_parallel_fcn31_matches_serial(h, w, name):
    launch(_worker, h * w, h, w, name, limit=240)
