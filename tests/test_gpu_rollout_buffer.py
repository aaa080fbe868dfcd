"""``makani_amd.rollout_buffer`` on the GPU against the fp64 restatement of tests/_rollout_ref.py.

Three successive updates with B = 2, 3, 1 go to lead time 1 of 3 (the first starts from n0 = 0, the last has zero batch M2; slots 0
and 2 stay exactly zero), on 9 x 14 (N = 126: one point per thread plus a tail, 8 orders, zonal tiles ragged in both directions),
17 x 32 (16-byte accesses) and 91 x 180 (several blocks per plane, partial last blocks), with all channels, with ["c3", "c0"] out
of order and with 6 of 7 (the padded row count of the transforms is then not the channel count), ensemble sizes 1, 2 and 4, f32 and
bf16 inputs, without and with scale / bias (bias / scale of order 1; one case with |bias| = 1e3 scale, compared at degree 0 /
order 0 separately from the rest).

Gate: relative L2 <= 1e-5 per output for ``running_mean``, ``running_var`` and the pair ``finalize()`` returns; 2^-8 for bf16 inputs,
whose rounded spectra may differ from the restatement's by one bf16 step.

The floor of the fp32 FORMULA on these inputs (the reference's op sequence in fp32 torch on the CPU against the same restatement,
tests/test_rollout_buffer.py::test_inputs_let_the_fp32_formula_meet_the_tolerance), worst case over the ten cases:
temporal mean 4.7e-8 / M2 3.8e-7, spectrum mean 2.3e-7 / M2 1.1e-6, zonal mean 1.7e-7 / M2 6.9e-7 (the M2 maxima are the
|bias| = 1e3 scale case, degree 0 / order 0 for the spectra; its other columns: mean 1.2e-7, M2 2.9e-7).  The f32 gate is 9 times
the worst of these, so it measures the kernels and not the conditioning of the inputs.  One more case, 25 channels with 4 members
(112 rows), makes the zonal kernel cut its rows into three tiles."""
import os
import sys
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rollout_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = ("temporal", "spectrum", "zonal")


@lru_cache(maxsize=None)
def _case(name):
    return R.case_setup(name)


@lru_cache(maxsize=None)
def _want(name, kind):
    c = _case(name)
    return R.restatement(kind, c["updates"], c["mask"], c["scale"], c["bias"], c["nlat"], c["nlon"], c["grid"])


def _make(kind, c, device=DEV):
    from makani_amd import rollout_buffer as rb
    common = dict(num_rollout_steps=R.T, rollout_dt=6, channel_names=R.names(c["nchan"]), device=device, scale=c["scale"], bias=c["bias"],
                  output_channels=c["selected"] if c["selected"] is not None else R.names(c["nchan"]))
    img = (c["nlat"], c["nlon"])
    lat_lon = (R.latitudes(c["nlat"]), R.longitudes(c["nlon"]))
    if kind == "temporal":
        return rb.TemporalAverageBuffer(img_shape=img, local_shape=img, local_offset=(0, 0), lat_lon=lat_lon, **common)
    if kind == "spectrum":
        return rb.SpectrumAverageBuffer(img_shape=img, ensemble_size=c["E"], grid_type=c["grid"], **common)
    return rb.ZonalSpectrumAverageBuffer(img_shape=img, ensemble_size=c["E"], lat_lon=lat_lon, **common)


def _update(buf, kind, data, targ, idt=R.IDT):
    if kind == "temporal":
        buf.update(data[:, 0].contiguous(), idt)
    else:
        buf.update(data, targ, idt)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_three_updates_equal_the_restatement(name, kind):
    c = _case(name)
    buf = _make(kind, c)
    for data, targ in c["updates"]:
        _update(buf, kind, data.to(DEV), targ.to(DEV))
    torch.cuda.synchronize()
    E1 = c["E"] + 1
    C = len(c["mask"])
    shape = {"temporal": (C, c["nlat"], c["nlon"]), "spectrum": (C, E1, c["nlat"]), "zonal": (C, E1, c["nlat"], c["nlon"] // 2 + 1)}[kind]
    assert tuple(buf.running_mean.shape) == tuple(buf.running_var.shape) == (R.T, *shape)
    assert buf.num_samples_tracked.flatten().tolist() == [0, sum(R.BATCHES), 0]
    for other in (0, 2):
        assert not buf.running_mean[other].any() and not buf.running_var[other].any()
    wmean, wm2, n = _want(name, kind)
    errs = {"mean": R.split_errors(kind, c["kind"], buf.running_mean[R.IDT], wmean),
            "m2": R.split_errors(kind, c["kind"], buf.running_var[R.IDT], wm2)}
    mean, std = buf.finalize()
    fmean, fstd = R.finalize_ref(wmean, wm2, n)
    errs["finalize mean"] = R.split_errors(kind, c["kind"], mean[R.IDT], fmean)
    errs["finalize std"] = R.split_errors(kind, c["kind"], std[R.IDT], fstd)
    print(f"{name} {kind}: " + " ".join(f"{k} {v}" for k, v in errs.items()))
    assert mean.dtype == std.dtype == torch.float32 and tuple(std.shape) == tuple(buf.running_var.shape)
    assert max(max(e.values()) for e in errs.values()) <= c["gate"], errs


@pytest.mark.parametrize("name", ["9x14-sel-e2-f32-unit", "17x32-6of7-e4-f32-unit", "17x32-sel-e2-f32-big", "91x180-sel-e2-bf16-unit",
                                  "17x32-all-e1-bf16-none"])
def test_power_spectrum_alone_equals_the_restatement(name):
    """the free function on (B, E, C, H, W): fp32 out whatever the input dtype, so f32's gate for both"""
    from makani_amd import rollout_buffer as rb
    from makani_amd.sht import RealSHT
    c = _case(name)
    data = c["updates"][1][0]                                                       # (3, E, C, H, W)
    sht = RealSHT(c["nlat"], c["nlon"], grid=c["grid"]).to(DEV)
    got = rb.power_spectrum(data.to(DEV), sht, c["scale"], c["bias"])
    x = data.double()
    if c["scale"] is not None:
        x = c["scale"].double()[None] * x + c["bias"].double()[None]
    p = torch.square(torch.abs(R.oracle_sht(c["nlat"], c["nlon"], c["grid"])(x)))
    p[..., 1:] *= 2.0
    want = p.sum(dim=-1)
    assert got.dtype == torch.float32 and tuple(got.shape) == (*data.shape[:3], c["nlat"])
    errs = R.split_errors("spectrum", c["kind"], got, want)
    print(f"power_spectrum {name}: {errs}")
    assert max(errs.values()) <= R.GATE_F32, errs
    one = rb.power_spectrum(data[0, 0].to(DEV), sht, c["scale"], c["bias"])         # (C, H, W): no leading dimension
    assert tuple(one.shape) == (data.shape[2], c["nlat"]) and R.rel(one, got[0, 0]) <= 1e-6
    with pytest.raises(ValueError):
        rb.power_spectrum(data[0, 0, 1].to(DEV), sht)                               # (H, W) has no channel axis


@pytest.mark.parametrize("kind", ["temporal", "spectrum"])
def test_an_update_replays_from_a_captured_graph(kind):
    """the sample count lives in device memory and ``update`` reads nothing back: one capture, three replays, the bits of three
    eager updates"""
    c = _case("17x32-all-e2-f32-unit")
    data, targ = (t.to(DEV) for t in c["updates"][0])
    eager, replayed = _make(kind, c), _make(kind, c)
    for _ in range(3):
        _update(eager, kind, data, targ)
    _update(replayed, kind, data, targ)                  # warms up outside the capture (library, FFT plan, one[l])
    replayed.zero_buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            _update(replayed, kind, data, targ)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert not replayed.num_samples_tracked.any() and not replayed.running_mean.any()       # a capture runs nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert replayed.num_samples_tracked.flatten().tolist() == [0, 3 * R.BATCHES[0], 0]
    assert torch.equal(replayed.num_samples_tracked, eager.num_samples_tracked)
    assert torch.equal(replayed.running_mean, eager.running_mean) and torch.equal(replayed.running_var, eager.running_var)
    assert eager.running_mean[R.IDT].any()
