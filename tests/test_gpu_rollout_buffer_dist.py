"""The rollout diagnostics on a sphere split over h x w ranks: processes sharing cuda:0 over gloo in the pattern of
tests/test_gpu_preproc_dist.py, each run under one time limit.  Grid 19 x 36: latitudes and degrees split [10, 9], orders [10, 9],
longitudes [18, 18].

* h2 w2: ``SpectrumAverageBuffer(spatial_distributed=True)`` holds this "h" rank's degrees; the shards put together equal the
  serial buffer within 1e-5 and the two "w" ranks of a row hold the same bits (the sums over the local orders are added over "w"
  before the statistics).  ``TemporalAverageBuffer`` with the shard's ``local_shape`` / ``local_offset`` equals the slice of the
  serial one.
* h2 w1: ``ZonalSpectrumAverageBuffer(spatial_distributed=True)`` equals the latitude slices of the serial buffer.
RCCL with more than one GPU is not exercised here."""
import pytest
import torch

from _ranks import launch, ranks

pytestmark = pytest.mark.gpu
IMG, NCHAN, SELECTED, E = (19, 36), 5, ["c3", "c0"], 2


def _worker(rank, world, rendezvous, h, w):
    with ranks(rank, world, rendezvous, timeout=120) as dist:
        import _rollout_ref as R
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        from makani_amd import rollout_buffer as rb
        dev = torch.device("cuda:0")
        scale, bias = R.affine("unit", NCHAN)
        updates = R.make_updates(*IMG, NCHAN, E, torch.float32, "unit", seed=77)
        common = dict(num_rollout_steps=R.T, rollout_dt=6, channel_names=R.names(NCHAN), device=dev, scale=scale, bias=bias,
                      output_channels=SELECTED)
        lat_lon = (R.latitudes(IMG[0]), R.longitudes(IMG[1]))

        def make(kind, local=None, offset=(0, 0), distributed=False):
            if kind == "temporal":
                return rb.TemporalAverageBuffer(img_shape=IMG, local_shape=local or IMG, local_offset=offset, lat_lon=lat_lon, **common)
            if kind == "spectrum":
                return rb.SpectrumAverageBuffer(img_shape=IMG, ensemble_size=E, grid_type="equiangular", spatial_distributed=distributed,
                                                **common)
            return rb.ZonalSpectrumAverageBuffer(img_shape=IMG, ensemble_size=E, lat_lon=lat_lon, spatial_distributed=distributed, **common)

        def run(buf, kind, cut):
            for data, targ in updates:
                data, targ = data[cut].contiguous().to(dev), targ[cut].contiguous().to(dev)
                if kind == "temporal":
                    buf.update(data[:, 0].contiguous(), R.IDT)
                else:
                    buf.update(data, targ, R.IDT)
            torch.cuda.synchronize()
            assert buf.num_samples_tracked.flatten().tolist() == [0, sum(R.BATCHES), 0]
            return buf.running_mean[R.IDT], buf.running_var[R.IDT]

        full = (Ellipsis, slice(None), slice(None))
        kinds = ("temporal", "spectrum") if w > 1 else ("temporal", "zonal")
        want = {k: run(make(k), k, full) for k in kinds}
        _, ih, iw = mcomm.init(h, w)
        assert thd.ensure_initialized()
        lat, lon = thd.compute_split_shapes(IMG[0], h), thd.compute_split_shapes(IMG[1], w)
        rows, cols = slice(sum(lat[:ih]), sum(lat[:ih + 1])), slice(sum(lon[:iw]), sum(lon[:iw + 1]))
        cut = (Ellipsis, rows, cols)
        errs = {}

        got = run(make("temporal", local=(lat[ih], lon[iw]), offset=(rows.start, cols.start)), "temporal", cut)
        for name, g, s in zip(("mean", "m2"), got, want["temporal"]):
            errs[f"temporal {name}"] = R.rel(g, s[cut])

        if w > 1:
            buf = make("spectrum", distributed=True)
            assert buf.spatial_distributed and (buf.lmax, buf.lmax_local, buf.lmax_offset) == (19, [10, 9][ih], [0, 10][ih])
            assert buf.sht.m_shapes == [10, 9] and tuple(buf.running_mean.shape) == (R.T, len(SELECTED), E + 1, buf.lmax_local)
            got = run(buf, "spectrum", cut)
            mine = torch.stack([torch.nn.functional.pad(t, (0, 10 - t.shape[-1])) for t in got]).cpu()      # shards padded to 10 degrees
            every = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            for i in range(h):                               # the "w" ranks of one row: the same bits
                assert all(torch.equal(every[i * w + j], every[i * w]) for j in range(w)), f"row {i}: the w ranks differ"
            whole = torch.cat([every[i * w][..., :[10, 9][i]] for i in range(h)], dim=-1)
            for k, name in enumerate(("mean", "m2")):
                errs[f"spectrum {name}"] = R.rel(whole[k], want["spectrum"][k])
                errs[f"spectrum {name} shard"] = R.rel(got[k], want["spectrum"][k][..., buf.lmax_offset:buf.lmax_offset + buf.lmax_local])
        else:
            buf = make("zonal", distributed=True)
            assert buf.spatial_distributed and (buf.nlat_local, buf.nlat_offset, buf.mmax_local) == (lat[ih], rows.start, 19)
            got = run(buf, "zonal", cut)
            for name, g, s in zip(("mean", "m2"), got, want["zonal"]):
                errs[f"zonal {name}"] = R.rel(g, s[..., rows, :])
        print(f"h{h}w{w} rank {rank}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
        assert max(errs.values()) <= 1e-5, (rank, errs)


def test_h2_w2_spectrum_shards_and_temporal_shards_equal_the_serial_buffers():
    launch(_worker, 4, 2, 2, limit=240)


def test_h2_w1_zonal_latitude_shards_equal_the_serial_buffer():
    launch(_worker, 2, 2, 1, limit=240)
