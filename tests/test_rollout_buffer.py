"""Host side of ``makani_amd.rollout_buffer``: the constructor contract of the three buffers, the transform of the constant field,
the pooling of the states of a process group, and the floor of the fp32 formula on the inputs of the GPU tests."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rollout_ref as R  # noqa: E402
from _ranks import launch, ranks  # noqa: E402

from makani_amd import rollout_buffer as rb  # noqa: E402

CPU = torch.device("cpu")
NAMES = R.names(5)
LATLON = (R.latitudes(9), R.longitudes(14))


def _temporal(**kw):
    args = dict(num_rollout_steps=3, rollout_dt=6, img_shape=(9, 14), local_shape=(9, 14), local_offset=(0, 0), channel_names=NAMES,
                lat_lon=LATLON, device=CPU, output_channels=NAMES)
    args.update(kw)
    return rb.TemporalAverageBuffer(**args)


def _spectrum(**kw):
    args = dict(num_rollout_steps=3, rollout_dt=6, img_shape=(9, 14), ensemble_size=2, grid_type="equiangular", channel_names=NAMES,
                device=CPU, output_channels=NAMES)
    args.update(kw)
    return rb.SpectrumAverageBuffer(**args)


def _zonal(**kw):
    args = dict(num_rollout_steps=3, rollout_dt=6, img_shape=(9, 14), ensemble_size=2, channel_names=NAMES, lat_lon=LATLON, device=CPU,
                output_channels=NAMES)
    args.update(kw)
    return rb.ZonalSpectrumAverageBuffer(**args)


def test_package_exports_the_buffers():
    import makani_amd as ma
    for n in ("MeanStdBuffer", "TemporalAverageBuffer", "SpectrumAverageBuffer", "ZonalSpectrumAverageBuffer", "power_spectrum"):
        assert n in ma.__all__ and getattr(ma, n) is getattr(rb, n)
    assert issubclass(rb.TemporalAverageBuffer, rb.MeanStdBuffer) and issubclass(rb.SpectrumAverageBuffer, rb.MeanStdBuffer)
    assert issubclass(rb.ZonalSpectrumAverageBuffer, rb.MeanStdBuffer)


def test_shapes_attributes_and_the_member_axis():
    t = _temporal(output_channels=["c3", "c0"], local_shape=(5, 14), local_offset=(4, 0))
    assert tuple(t.running_mean.shape) == tuple(t.running_var.shape) == (3, 2, 5, 14)
    assert t.running_mean.dtype == t.running_var.dtype == torch.float32
    assert tuple(t.num_samples_tracked.shape) == (3, 1, 1, 1) and t.num_samples_tracked.dtype == torch.int64
    assert t.channel_mask == [3, 0] and t.num_channels == 2 and t.variable_dims == 2
    assert tuple(t.scale.shape) == tuple(t.bias.shape) == (1, 2, 1, 1)
    assert torch.equal(t.scale.flatten(), torch.ones(2)) and torch.equal(t.bias.flatten(), torch.zeros(2))
    assert (t.img_shape, t.local_shape, t.local_offset, t.rollout_dt, t.num_rollout_steps) == ((9, 14), (5, 14), (4, 0), 6, 3)

    scale, bias = R.affine("unit", 5)
    s = _spectrum(scale=scale, bias=bias, output_channels=["c3", "c0"])
    assert tuple(s.running_mean.shape) == (3, 2, 3, 9)                     # E1 = ensemble_size + 1 on ensemble rank 0
    assert tuple(s.num_samples_tracked.shape) == (3, 1, 1, 1)
    assert (s.lmax, s.lmax_local, s.lmax_offset, s.ensemble_size, s.spatial_distributed) == (9, 9, 0, 2, False)
    assert tuple(s.scale.shape) == (1, 1, 2, 1, 1)
    assert torch.equal(s.scale.flatten(), scale.flatten()[[3, 0]]) and torch.equal(s.bias.flatten(), bias.flatten()[[3, 0]])

    z = _zonal(ensemble_size=4)
    assert tuple(z.running_mean.shape) == (3, 5, 5, 9, 8)
    assert tuple(z.num_samples_tracked.shape) == (3, 1, 1, 1, 1)
    assert (z.mmax, z.mmax_local, z.mmax_offset, z.nlat_local, z.nlat_offset, z.nlat) == (8, 8, 0, 9, 0, 9)
    assert tuple(z.lat_weights.shape) == (1, 1, 1, 9, 1)
    assert torch.allclose(z.lat_weights.flatten(), R.lat_weights(9))

    for b in (t, s, z):
        b.running_mean.fill_(1.0), b.running_var.fill_(2.0), b.num_samples_tracked.fill_(3)
        b.zero_buffers()
        assert not b.running_mean.any() and not b.running_var.any() and not b.num_samples_tracked.any()


def test_other_ensemble_ranks_hold_no_truth(monkeypatch):
    from makani_amd import comm
    monkeypatch.setitem(comm._GROUPS, "ensemble", (None, 2, 1))
    assert tuple(_spectrum().running_mean.shape) == (3, 5, 2, 9)
    assert tuple(_zonal().running_mean.shape) == (3, 5, 2, 9, 8)


def test_refused_configurations(monkeypatch):
    for make in (_temporal, _spectrum, _zonal):
        with pytest.raises(ValueError, match="Empty channel lists"):
            make(output_channels=[])
        with pytest.raises(NotImplementedError):
            make(output_file="stats.h5")
        with pytest.raises(ValueError):
            make(output_channels=["nope"])
    x = torch.zeros(2, 5, 9, 14)
    with pytest.raises(RuntimeError):
        _temporal().update(x, 0)
    with pytest.raises(RuntimeError):
        _spectrum().update(x[:, None].expand(2, 2, 5, 9, 14), x[:, None], 0)
    with pytest.raises(RuntimeError):
        _zonal().update(x[:, None].expand(2, 2, 5, 9, 14), x[:, None], 0)
    with pytest.raises(RuntimeError):
        rb.power_spectrum(x, _spectrum().sht)
    from makani_amd import comm
    for name, size in (("spatial", 4), ("h", 2), ("w", 2)):
        monkeypatch.setitem(comm._GROUPS, name, (None, size, 0))
    monkeypatch.setattr(comm, "_SOURCE", "init")
    with pytest.raises(NotImplementedError, match="'w'"):
        _zonal(spatial_distributed=True)
    monkeypatch.setitem(comm._GROUPS, "w", (None, 1, 0))
    monkeypatch.setitem(comm._GROUPS, "h", (None, 2, 1))
    z = _zonal(spatial_distributed=True)
    assert (z.nlat_local, z.nlat_offset) == (4, 5) and tuple(z.running_mean.shape) == (3, 5, 3, 4, 8)
    assert torch.allclose(z.lat_weights.flatten(), R.lat_weights(9)[5:])


@pytest.mark.parametrize("nlat,nlon,grid", [(9, 14, "equiangular"), (17, 32, "legendre-gauss"), (91, 180, "equiangular"),
                                            (19, 36, "equiangular")])
def test_constant_field_coefficients_equal_the_oracle_transform(nlat, nlon, grid):
    from makani_amd.sht import RealSHT
    one = rb.constant_field_coefficients(RealSHT(nlat, nlon, grid=grid))
    want = R.oracle_sht(nlat, nlon, grid)(torch.ones(nlat, nlon, dtype=torch.float64))
    assert one.dtype == np.float64 and one.shape == (nlat,)
    assert np.abs(one - want[:, 0].real.numpy()).max() <= 1e-13
    assert want[:, 1:].abs().max() <= 1e-13 and want[:, 0].imag.abs().max() <= 1e-13
    # both rules integrate the degrees below nlat exactly: sqrt(4 pi) at l = 0 and rounding noise elsewhere
    assert abs(one[0] - np.sqrt(4 * np.pi)) <= 1e-12 and np.abs(one[1:]).max() <= 1e-13


def _pool_worker(rank, world, rendezvous, out):
    with ranks(rank, world, rendezvous, timeout=60):
        import makani_amd.comm as mcomm
        mcomm.init(1, 1)
        assert mcomm.get_size("batch") == 2 and mcomm.get_size("data") == 2
        g = torch.Generator().manual_seed(5)
        samples = torch.randn((7, 5, 3, 9), generator=g, dtype=torch.float64) * 2.0 + 3.0        # rank 0: 3 samples, rank 1: 4
        mine = samples[:3] if rank == 0 else samples[3:]
        for buf, group in ((_spectrum(), "batch"), (_temporal(local_shape=(3, 9)), "data")):
            buf.running_mean[1] = mine.mean(0).float()
            buf.running_var[1] = torch.square(mine - mine.mean(0)).sum(0).float()
            buf.num_samples_tracked[1] = mine.shape[0]
            buf.running_mean[0] = float(rank + 1)              # slot 0: one sample per rank, values 1 and 2
            buf.num_samples_tracked[0] = 1
            buf._aggregate_stats(group)
            assert buf.num_samples_tracked.flatten().tolist() == [2, 7, 0]
            want_mean = samples.mean(0)
            want_m2 = torch.square(samples - want_mean).sum(0)
            assert R.rel(buf.running_mean[1], want_mean) <= 1e-6 and R.rel(buf.running_var[1], want_m2) <= 1e-6
            assert torch.equal(buf.running_mean[0], torch.full_like(buf.running_mean[0], 1.5))
            assert torch.allclose(buf.running_var[0], torch.full_like(buf.running_var[0], 0.5))
            mean, std = buf.finalize()                         # pools once more: every rank now holds the pooled state
            assert mean is buf.running_mean and buf.num_samples_tracked.flatten().tolist() == [4, 14, 0]
        if rank == 0:
            open(out, "w").write("ok")


def test_two_ranks_pool_to_the_statistics_of_all_samples(tmp_path):
    out = str(tmp_path / "ok")
    launch(_pool_worker, 2, out, limit=120)
    assert os.path.exists(out)


def test_finalize_of_one_sample_is_not_finite():
    t = _temporal()
    t.running_mean[0] = 2.0
    t.running_var[0] = 1.0
    t.num_samples_tracked[0] = 1
    t.num_samples_tracked[1] = 1
    mean, std = t.finalize()
    # sqrt of 1 / 0, of 0 / 0 and (an empty slot) of 0 / -1 = -0
    assert torch.isinf(std[0]).all() and torch.isnan(std[1]).all() and not std[2].any()
    assert torch.equal(mean[0], torch.full_like(mean[0], 2.0))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_inputs_let_the_fp32_formula_meet_the_tolerance(name):
    """The reference's own op sequence in fp32 torch on the CPU (oracle SHT, ``torch.fft.rfft``, ``var_mean``,
    ``_welford_combine``) against the fp64 restatement on the GPU tests' inputs: within the GPU gate for mean AND M2 of every
    buffer.  The gate of tests/test_gpu_rollout_buffer.py therefore measures the kernels, not the conditioning of the inputs."""
    c = R.case_setup(name)
    for kind in ("temporal", "spectrum", "zonal"):
        args = (kind, c["updates"], c["mask"], c["scale"], c["bias"], c["nlat"], c["nlon"], c["grid"])
        mean, m2, n = R.reference_sequence(*args)
        wmean, wm2, wn = R.restatement(*args)
        assert n == wn == sum(R.BATCHES)
        errs = {"mean": R.split_errors(kind, c["kind"], mean, wmean), "m2": R.split_errors(kind, c["kind"], m2, wm2)}
        print(f"fp32 formula {name} {kind}: {errs}")
        assert max(max(e.values()) for e in errs.values()) <= c["gate"], (kind, errs)
