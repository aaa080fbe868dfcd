"""Time one ``update`` of each rollout diagnostic buffer (makani_amd/rollout_buffer.py) beside the torch composition of the
reference's sequence (makani/utils/inference/rollout_buffer.py:919-931, 1037-1079, 1284-1320) on the same GPU.

The composition uses THIS package's transforms (``RealSHT.forward``, ``ops.rfft_rows`` turned into the complex (B, E1, C, H, M)
tensor the reference's ``rfft`` returns), so the two columns differ in what the buffers replace — the concatenation, the channel
gather, ``scale * x + bias``, ``|c|^2``, the permuted copy, ``var_mean`` and the combine with its host read of the count — and
not in the transform.  The transform alone is timed as well.

Sizes: 721 x 1440 x 73 and 240 x 480 x 73, B = 2, ``ensemble_size`` = 1, fp32, scale and bias given.  Device events around a window
of at least ``--iters`` calls and ``--min-window-ms`` of work after ``--warmup`` calls, the median of ``--repeats`` such windows;
the buffers and the composition are timed in turn inside every repeat.  For the two streaming kernels (``mk_welford_update`` as the temporal update, ``mk_zonal_welford`` on a ready F) the
algorithmic bytes and their share of the 8 TB/s HBM peak are printed.  No GPU: the script fails, it has no fallback.

    python tools/rollout_buffer_bench.py [--out FILE] [--sizes 721x1440,240x480] [--iters 10] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fns, warmup, iters, repeats, min_window_ms):
    """{name: (median ms per call, calls per window)}; the functions take turns inside every repeat; a window holds at least
    ``iters`` calls and at least ``min_window_ms`` of work (sized from a first short window)"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    calls = {k: max(iters, min(5000, int(min_window_ms / max(window(fn, 3), 1e-4)) + 1)) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, calls[k]))
    return {k: (statistics.median(v), calls[k]) for k, v in times.items()}


class TorchComposition:
    """the reference's op sequence on torch tensors, state and count as the reference keeps them"""

    def __init__(self, shape, scale, bias, dev):
        self.mean = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.m2 = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.count = torch.zeros((1,) * len(shape), dtype=torch.int64, device=dev)
        self.scale, self.bias = scale, bias

    def combine(self, y):
        count = torch.tensor(y.shape[0], dtype=torch.int64, device=y.device).reshape(self.count.shape)
        var, mean = torch.var_mean(y, dim=0, correction=0, keepdim=False)
        m2 = var * count
        new = self.count + count
        delta = mean - self.mean
        self.mean += delta * float(count) / float(new)                                 # two host reads of device values
        self.m2 += m2 + torch.square(delta) * float(self.count * count) / float(new)
        self.count[...] = new


def run_size(H, W, C, B, E, args, dev):
    from makani_amd import ops, rollout_buffer as rb
    from makani_amd._lib import check, lib, ptr, stream
    names = [f"c{i}" for i in range(C)]
    g = torch.Generator().manual_seed(0)
    data = torch.randn((B, E, C, H, W), generator=g).to(dev)
    targ = torch.randn((B, 1, C, H, W), generator=g).to(dev)
    scale = (0.5 + torch.rand(C, generator=g)).reshape(1, C, 1, 1)
    bias = torch.randn(C, generator=g).reshape(1, C, 1, 1)
    lat_lon = (torch.linspace(90, -90, H).tolist(), torch.linspace(0, 360, W + 1)[:-1].tolist())
    common = dict(num_rollout_steps=1, rollout_dt=6, channel_names=names, device=dev, scale=scale, bias=bias, output_channels=names)
    tb = rb.TemporalAverageBuffer(img_shape=(H, W), local_shape=(H, W), local_offset=(0, 0), lat_lon=lat_lon, **common)
    sb = rb.SpectrumAverageBuffer(img_shape=(H, W), ensemble_size=E, grid_type="equiangular", **common)
    zb = rb.ZonalSpectrumAverageBuffer(img_shape=(H, W), ensemble_size=E, lat_lon=lat_lon, **common)
    E1, M, L = E + 1, W // 2 + 1, sb.lmax
    s5, b5 = scale.to(dev).reshape(1, 1, C, 1, 1), bias.to(dev).reshape(1, 1, C, 1, 1)
    x4 = data[:, 0].contiguous()
    Cp = ops.round4(C)
    fw = (1.0 / W,) * 3

    t_ref = TorchComposition((C, H, W), scale.to(dev), bias.to(dev), dev)
    s_ref = TorchComposition((C, E1, L), s5, b5, dev)
    z_ref = TorchComposition((C, E1, H, M), s5, b5, dev)
    latw = zb.lat_weights

    def torch_temporal():
        t_ref.combine(t_ref.scale * x4 + t_ref.bias)

    def torch_spectrum():
        x = s_ref.scale * torch.cat([targ, data], dim=1) + s_ref.bias
        p = torch.square(torch.abs(sb.sht(x)))
        p[..., 1:] *= 2.0
        s_ref.combine(torch.sum(p, dim=-1).permute(0, 2, 1, 3).contiguous())

    def package_rfft(x):                                       # (B, E1, C, H, W) -> complex (B, E1, C, H, M), norm="forward"
        F = ops.rfft_rows(x.reshape(-1, C, H, W), M, Cp, fw)
        return torch.view_as_complex(F.view(M, H, 2, B, E1, Cp)[..., :C].permute(3, 4, 5, 1, 0, 2).contiguous())

    def torch_zonal():
        x = z_ref.scale * torch.cat([targ, data], dim=1) + z_ref.bias
        p = latw * torch.square(torch.abs(package_rfft(x)))
        p[..., 1:] *= 2.0
        z_ref.combine(p.permute(0, 2, 1, 3, 4).contiguous())

    both = torch.cat([targ, data], dim=1)
    F_members = ops.rfft_rows(data.reshape(-1, C, H, W), M, Cp, fw)

    def zonal_kernel():
        check(lib().mk_zonal_welford(ptr(F_members), ptr(zb._scale), ptr(zb._bias), ptr(zb._latw), ptr(zb.running_mean[0]),
                                     ptr(zb.running_var[0]), ptr(zb.num_samples_tracked[0]), 0, M, H, F_members.shape[3], Cp, B, E, C, E1,
                                     1, stream()), "mk_zonal_welford")

    fns = {
        "temporal update": lambda: tb.update(x4, 0),
        "temporal torch": torch_temporal,
        "spectrum update": lambda: sb.update(data, targ, 0),
        "spectrum torch": torch_spectrum,
        "spectrum transform alone": lambda: sb.sht.analysis(both.reshape(-1, C, H, W)),
        "zonal update": lambda: zb.update(data, targ, 0),
        "zonal torch": torch_zonal,
        "zonal transform alone": lambda: ops.rfft_rows(both.reshape(-1, C, H, W), M, Cp, fw),
        "zonal kernel alone (members)": zonal_kernel,
    }
    timed = measure(fns, args.warmup, args.iters, args.repeats, args.min_window_ms)
    ms = {k: v[0] for k, v in timed.items()}
    n = C * H * W
    nbytes = {"temporal update": (B + 4) * n * 4,                                           # the batch once, mean and M2 read and written
              "zonal kernel alone (members)": (2 * B * E + 4 * E) * C * H * M * 4}            # F (re, im) once, the members' mean and M2
    rows = []
    for k, v in ms.items():
        row = dict(size=f"{H}x{W}x{C}", B=B, E=E, what=k, ms=round(v, 4), calls_per_window=timed[k][1])
        if k in nbytes:
            row["GB"] = round(nbytes[k] / 1e9, 4)
            row["hbm_peak_share"] = round(nbytes[k] / (v * 1e-3) / HBM_PEAK, 3)
        rows.append(row)
    for kind in ("temporal", "spectrum", "zonal"):
        rows.append(dict(size=f"{H}x{W}x{C}", B=B, E=E, what=f"{kind} torch / update", ratio=round(ms[f"{kind} torch"] / ms[f"{kind} update"], 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="721x1440,240x480")
    ap.add_argument("--channels", type=int, default=73)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--ensemble", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-window-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_buffer_bench needs a GPU: timings are taken on the device or not at all")
    dev = torch.device("cuda:0")
    lines = []
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        with torch.no_grad():
            for row in run_size(H, W, args.channels, args.batch, args.ensemble, args, dev):
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
