"""The cosine solar zenith angle on the GPU (csrc/zenith.hip behind ``makani_amd.zenith``) against the fp64 restatement
tests/_zenith_ref.py.

Grids (poles on the grid): 5 x 9 (one pixel per lane only), 33 x 64 (16-byte stores, five row tiles, the last one of one row),
91 x 180 (twelve row tiles, the last one of three rows).  Times: _zenith_ref.TIMES.  Gate, f32: 2e-6 absolute.  The four tables
and the four time scalars are fp64 values rounded once to fp32, and a pixel is five fp32 operations on values <= 1 behind them:
at most ten half-ulps of 1 = 6e-7, three times over.  bf16: the f32 result rounded to bf16, bit for bit.  Strided destinations,
shards and graph replays: bit for bit the contiguous / serial / eager planes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _zenith_ref as ref          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRIDS = [(5, 9), (33, 64), (91, 180)]
HOUR = 3_600_000_000
T0 = ref.times_us()
# name -> (B, times (Bt, T))
WINDOWS = {"1x1": (1, T0[3:].reshape(1, 1)),
           "2x3": (2, np.concatenate([T0, T0[:2] + HOUR]).reshape(2, 3)),
           "shared": (2, T0[[0, 2]].reshape(1, 2))}


def _grid(H, W):
    return np.linspace(90.0, -90.0, H), np.linspace(0.0, 360.0, W, endpoint=False)


def _module(H, W, times, dtype=torch.float32, **kw):
    import makani_amd as ma
    lat, lon = _grid(H, W)
    z = ma.ZenithFeatures(lat, lon, n_history=times.shape[1] - 1, dtype=dtype, **kw).to(DEV)
    return z.set_time(torch.from_numpy(times).to(DEV), batch_size=times.shape[0])


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("H,W", GRIDS)
def test_planes_against_fp64(H, W, window):
    B, times = WINDOWS[window]
    got = _module(H, W, times)(B)
    assert got.shape == (B, times.shape[1], H, W) and got.dtype == torch.float32
    want = np.broadcast_to(ref.cos_zenith(times, *_grid(H, W)), got.shape)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"{H} x {W} {window}: max |f32 - fp64| = {err:.3e}")
    assert err <= 2e-6
    half = _module(H, W, times, dtype=torch.bfloat16)(B)
    assert half.dtype == torch.bfloat16 and torch.equal(_bits(half), _bits(got.to(torch.bfloat16)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_offset"])
def test_channel_slots_of_a_larger_buffer(offset, dtype):
    H, W = 33, 64
    B, times = WINDOWS["2x3"]
    z = _module(H, W, times[:, :2], dtype=dtype)
    dense = z(B)
    flat = torch.full((B * 9 * H * W + 2,), 7.0, dtype=dtype, device=DEV)
    buf = flat[offset:offset + B * 9 * H * W].view(B, 9, H, W)
    out = z(B, out=buf[:, 3::4])
    assert out.data_ptr() == buf[0, 3].data_ptr() and torch.equal(_bits(buf[:, [3, 7]]), _bits(dense))
    buf[:, [3, 7]] = 7.0
    assert bool((flat == 7.0).all())


@pytest.mark.parametrize("rows,cols", [([17, 16], [36, 28]), ([17, 16], [33, 31]), ([12, 11, 10], [64])], ids=["2x2", "2x2_odd", "3x1"])
def test_a_shard_is_the_slice_of_the_serial_plane(rows, cols):
    import makani_amd as ma
    B, times = WINDOWS["2x3"]
    serial = _module(33, 64, times)(B)
    lat, lon = _grid(33, 64)
    r0 = 0
    for nr in rows:
        c0 = 0
        for nc in cols:
            z = ma.ZenithFeatures(lat[r0:r0 + nr], lon[c0:c0 + nc], n_history=2).to(DEV)
            z.set_time(torch.from_numpy(times).to(DEV), batch_size=B)
            assert torch.equal(z(B), serial[:, :, r0:r0 + nr, c0:c0 + nc]), (r0, c0)
            c0 += nc
        r0 += nr


def test_graph_replays_step_the_valid_time_on_the_device():
    H, W = 33, 64
    B, times = WINDOWS["2x3"]
    eager = [_module(H, W, times + k * 6 * HOUR)(B) for k in range(3)]
    z = _module(H, W, times, dt_hours=6)
    start = z.times.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):          # warm-up outside the capture: builds the tables
        z(B)
        z.advance()
    torch.cuda.synchronize()
    z.times.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = z(B)
        z.advance()
    torch.cuda.synchronize()
    got = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            graph.replay()
            got.append(out.clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in range(3):
        assert torch.equal(got[k], eager[k]), k
    assert torch.equal(z.times, start + 3 * 6 * HOUR)


def test_time_layouts_of_the_model_package():
    import makani_amd as ma
    H, W = 5, 9
    lat, lon = _grid(H, W)
    stamps = np.array(ref.TIMES, dtype="datetime64[us]")
    z = ma.ZenithFeatures(lat, lon, n_history=1).to(DEV)
    per_member = z.set_time(stamps, batch_size=2)(2)                  # 2 * 2 times, member-major
    assert z.times.shape == (2, 2) and per_member.shape == (2, 2, H, W)
    shared = z.set_time(stamps[:2], batch_size=2)(2)                  # one window for both members
    assert z.times.shape == (1, 2) and shared.shape == (2, 2, H, W)
    assert torch.equal(shared[0], per_member[0]) and torch.equal(shared[1], per_member[0])
    # the functional form on host datetimes and the reference's 2-D meshgrid: the same planes
    assert torch.equal(ma.cos_zenith_angle(stamps, *np.meshgrid(lon, lat), device=DEV), per_member.reshape(4, H, W))
    with pytest.raises(ValueError, match=r"add_zenith: got 3 time\(s\) for a batch of 2 with n_history=1\. Pass either 4 times"):
        z.set_time(stamps[:3], batch_size=2)
    for call in (lambda t: z.set_time(t[:2], batch_size=2), lambda t: ma.cos_zenith_angle(t, lon, lat)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(torch.from_numpy(ref.times_us()))
