"""bench.py — SFNO train-step throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

One "step" = forward + backward + gradient clipping + AdamW update of
``sfno_sc3_layers8_edim384`` (config/sfnonet.yaml: scale_factor 3, 8 layers, embed_dim 384,
dhconv, instance norm, mlp_ratio 2) at 721 x 1440, 73 -> 73 channels, batch 1 per GPU,
bf16 autocast (fp32 spectral path), synthetic DummyLoader-shaped data resident in HBM.
N > 1: one process per GPU over RCCL.  Launched either by the driver through ``torch.distributed.run`` (RANK /
WORLD_SIZE / MASTER_* in the environment) or directly as ``python bench.py --gpus N`` (the script then spawns its N
ranks itself).  The headline measurement at N > 1 is the north-star split — spatial model parallelism h x w over ALL N
GPUs (N = 4: h4w1, 8: h4w2; "scaling": "strong", one sample per step) — and the same run then measures plain
data parallelism (one sample per GPU, gradient all-reduce overlapped with backward, "weak") as ``secondary``.  At N = 2 the
headline IS data parallelism (the reference's partitioning has no 2-GPU split worth running on xGMI: default_parallelism).
``--parallelism dp|hHwW`` picks the headline explicitly.

A plain run sets up, warms up, times the K steps and prints the headline.  ``--full`` adds everything else the line can
carry: per-kernel table and roofline, the step with exact fp32 spectral arithmetic, forward SHT bandwidth, CPU baseline,
in-run parity against the oracle and, at N > 1, the exchange volume and the data-parallel ``secondary``.
``--dump-outputs DIR`` writes what the last timed step computed as DIR/<name>.npy (``dump_outputs``).

Rank 0 prints ONE JSON line (see DESIGN.md §7 for every field).
"""
import argparse
import json
import math
import os
import sys
import time

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver (already exported on the boxes)
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

CONFIGS = {
    # BASELINE.json configs[1]
    "sfno_sc3_layers8_edim384": dict(inp_shape=(721, 1440), out_shape=(721, 1440), inp_chans=73, out_chans=73,
                                     scale_factor=3, embed_dim=384, num_layers=8, mlp_ratio=2, operator_type="dhconv",
                                     normalization_layer="instance_norm", activation_function="gelu", big_skip=True,
                                     model_grid_type="equiangular", sht_grid_type="legendre-gauss"),
    # small stand-in with the same structure (plumbing / CI on small GPUs)
    "sfno_debug": dict(inp_shape=(91, 180), out_shape=(91, 180), inp_chans=8, out_chans=8, scale_factor=3,
                       embed_dim=64, num_layers=4, mlp_ratio=2),
    # ... on a grid whose row lengths (1440 / 480) have specialised FFT kernels, so that an h x w split of it runs the FUSED
    # exchange schedule of makani_amd/dist_pipeline.py like the headline config does (plumbing / CI of the N > 1 line)
    "sfno_debug_seg": dict(inp_shape=(91, 1440), out_shape=(91, 1440), inp_chans=8, out_chans=8, scale_factor=3,
                           embed_dim=32, num_layers=2, mlp_ratio=2),
}
_LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
_FCN3_CHANS = ["u10m", "v10m", "u100m", "v100m", "t2m", "msl", "tcwv"] + [f"{v}{l}" for v in "uvztq" for l in _LEVELS]
# auxiliary channels as makani's driver names them (makani/utils/features.py:20-67; driver.py:212-263): zenith angle, the 8
# concatenated noise channels of the ensemble recipe (config/fourcastnet3.yaml:165-172), orography, the two land-sea masks
_FCN3_AUX = ["xzen"] + [f"xnoise{i}" for i in range(8)] + ["xoro", "xlsml", "xlsms"]
# BASELINE.json configs[3]: fcn3_sc2_edim45_layers10 (config/fourcastnet3.yaml:24-46), trained with the ensemble recipe of its
# second pre-training stage (:174-202,254-262): ensemble_size 2, loss = fair CRPS ("skillspread") + 0.1 x spectral CRPS.
# One sample = one initial condition = ensemble_size forward passes (the members are the model's batch).
FCN3_CONFIGS = {
    "fcn3_sc2_edim45_layers10": dict(
        ensemble_size=2, lr=4e-4,
        model=dict(inp_shape=(721, 1440), out_shape=(721, 1440), scale_factor=2, model_grid_type="equiangular",
                   sht_grid_type="legendre-gauss", filter_basis_type="morlet", kernel_shape=(3, 3), channel_names=_FCN3_CHANS,
                   aux_channel_names=_FCN3_AUX, atmo_embed_dim=45, surf_embed_dim=56, aux_embed_dim=36, num_layers=10,
                   sfno_block_frequency=5, num_groups=1, normalization_layer="none", hard_thresholding_fraction=1.0, use_mlp=True,
                   mlp_ratio=2, activation_function="gelu", big_skip=False, bias=False, encoder_mlp=False)),
    # the same network on a small grid with few variables (plumbing / CI)
    "fcn3_debug": dict(
        ensemble_size=2, lr=4e-4,
        model=dict(inp_shape=(65, 128), out_shape=(65, 128), scale_factor=2, filter_basis_type="morlet", kernel_shape=(3, 3),
                   channel_names=["u10m", "t2m", "u500", "t500", "u850", "t850"], aux_channel_names=["xzen", "xnoise0", "xoro"],
                   atmo_embed_dim=8, surf_embed_dim=8, aux_embed_dim=6, num_layers=4, sfno_block_frequency=2,
                   normalization_layer="none", use_mlp=True, mlp_ratio=2, big_skip=False)),
}
for _k, _v in FCN3_CONFIGS.items():
    CONFIGS[_k] = dict(kind="fcn3", inp_shape=_v["model"]["inp_shape"], out_shape=_v["model"]["out_shape"],
                       inp_chans=len(_v["model"]["channel_names"]) + len(_v["model"]["aux_channel_names"]),
                       out_chans=len(_v["model"]["channel_names"]), **_v)
PMC_TRAFFIC = "r06_pmc_hbm_traffic.json"              # written by tools/profile_round.sh on this round's code (fallback of the live passes)
PMC_TRAFFIC_FCN3 = "r06_pmc_hbm_traffic_fcn3.json"
PEAK_F32_VALU_TF = 157.3      # packed fp32 FMA on the vector ALUs (MI355X_MICROARCH.md)
PEAK_F32_MFMA_TF = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md
PEAK_BF16_MFMA_TF = 2500.0    # dense
PEAK_HBM_GBS = 8000.0


def make_loss(H, W, channels, device, spatial):
    """The config's training loss (config/sfnonet.yaml:43-48: type "l2", squared): GeometricLpLoss(p=2, squared=True)
    on the equiangular grid (makani/utils/losses/lp_loss.py:28-107), uniform channel weights, mean over (B, C) —
    on the HIP path (makani_amd.GeometricLpLoss: one fused kernel forward, one backward)."""
    import makani_amd as ma
    fn = ma.GeometricLpLoss(img_shape=(H, W), crop_shape=(H, W), crop_offset=(0, 0),
                            channel_names=[f"c{i}" for i in range(channels)], p=2.0, squared=True,
                            grid_type="equiangular", spatial_distributed=spatial).to(device)
    return lambda pred, tar: fn(pred, tar).mean()


def kernel_family(name):
    """Launch names of the channel GEMMs carry their shape (``conv1x1_wgrad_m384_k768_n115200``): one kernel symbol,
    nine shapes per step.  The family is what rocprofv3 aggregates under one kernel name."""
    import re
    name = re.sub(r"_\d+x\d+_p\d+$", "", name)          # disco_fwd_360x720_p1354 -> disco_fwd
    return re.sub(r"_m\d+_k\d+_n\d+$", "", name)


def dominant_family(summary):
    """(family, member launch names) with the largest accumulated time in a LaunchProfiler summary"""
    fam = {}
    for k, d in summary.items():
        fam.setdefault(kernel_family(k), []).append(k)
    if not fam:
        return None, []
    best = max(fam, key=lambda f: sum(summary[k]["ms_total"] for k in fam[f]))
    return best, sorted(fam[best])


def kernel_table(warm_prof, prof, steps):
    """per launch name: launches/step, mean duration, ms/step, dense TFLOP/s, algorithmic GB/s.  Numbers come from the
    timed region where a kernel was instrumented there, else from the fully profiled last warm-up step."""
    table, table_steps = (warm_prof, 1) if warm_prof else (prof, steps)
    kernels = {}
    for k, d in sorted(table.items(), key=lambda kv: -kv[1]["ms_total"]):
        nsteps = table_steps
        if k in prof:
            d, nsteps = prof[k], steps
        tf = d["flops"] / d["launches"] / (d["ms_avg"] * 1e-3) / 1e12 if d["flops"] else None
        gb = d["bytes"] / d["launches"] / (d["ms_avg"] * 1e-3) / 1e9
        kernels[k] = dict(launches_per_step=d["launches"] / nsteps, ms_avg=round(d["ms_avg"], 4),
                          ms_per_step=round(d["ms_total"] / nsteps, 3),
                          TFLOPs_dense=round(tf, 2) if tf else None, GBps_algorithmic=round(gb, 1))
    return kernels


def roofline_of(family, members, prof, gemm_mode, traffic):
    """The ``roofline`` object for one kernel family: algorithmic flops / bytes per launch (summed over the family's
    launches in ``prof``) over its mean launch duration.  Bound: HBM for kernels without matrix work; for the bf16
    channel GEMMs whichever roof the shape mix sits under (arithmetic intensity vs 2500 TF / 8 TB/s = 312 flop/B);
    the fp32 spectral GEMMs are priced against the matrix rate of the engine they run on."""
    ds = [prof[m] for m in members if m in prof]
    launches = sum(d["launches"] for d in ds)
    if not launches:
        return None
    ms_avg = sum(d["ms_total"] for d in ds) / launches
    flops = sum(d["flops"] for d in ds) / launches
    nbytes = sum(d["bytes"] for d in ds) / launches
    tf = flops / (ms_avg * 1e-3) / 1e12
    gb = nbytes / (ms_avg * 1e-3) / 1e9
    base = dict(kernel=family, launches=launches, ms_avg=round(ms_avg, 4), algorithmic_bytes=int(nbytes),
                algorithmic_flops=int(flops), traffic=traffic)
    if len(members) > 1:
        base["shapes"] = members
    if not flops:
        return dict(base, bound="hbm", achieved=round(gb, 1), peak=PEAK_HBM_GBS, unit="GB/s", frac=round(gb / PEAK_HBM_GBS, 4))
    if family.startswith(("disco", "resample", "group_mix")):
        # sliding-window contractions on the vector ALUs (no matrix-core shape): priced against the packed-fp32 FMA peak when
        # their arithmetic intensity is above the VALU ridge (157.3 TF / 8 TB/s = 20 flop/B), else against HBM
        if flops / (PEAK_F32_VALU_TF * 1e12) >= nbytes / (PEAK_HBM_GBS * 1e9):
            return dict(base, bound="valu", achieved=round(tf, 2), peak=PEAK_F32_VALU_TF, unit="TFLOP/s",
                        frac=round(tf / PEAK_F32_VALU_TF, 4), GBps=round(gb, 1),
                        note="fp32 multiply-adds of the convolution tensor's entries (2 x nnz x planes x longitudes) on the "
                             "vector ALUs against the packed-FMA peak; no MFMA shape exists for a sparse circular correlation")
        return dict(base, bound="hbm", achieved=round(gb, 1), peak=PEAK_HBM_GBS, unit="GB/s", frac=round(gb / PEAK_HBM_GBS, 4),
                    TFLOPs=round(tf, 1))
    if family.startswith("conv1x1"):
        if flops / (PEAK_BF16_MFMA_TF * 1e12) < nbytes / (PEAK_HBM_GBS * 1e9):      # below the ridge: HBM is the roof
            return dict(base, bound="hbm", achieved=round(gb, 1), peak=PEAK_HBM_GBS, unit="GB/s",
                        frac=round(gb / PEAK_HBM_GBS, 4), TFLOPs=round(tf, 1),
                        note=f"bf16 channel GEMM, {flops / nbytes:.0f} flop/B < 312 flop/B ridge: HBM-bound; "
                             f"{tf:.0f} TF = {tf / PEAK_BF16_MFMA_TF:.3f} of the bf16 MFMA peak")
        return dict(base, bound="mfma", achieved=round(tf, 2), peak=PEAK_BF16_MFMA_TF, unit="TFLOP/s",
                    frac=round(tf / PEAK_BF16_MFMA_TF, 4), GBps=round(gb, 1), note="bf16 MFMA")
    peak, eng = {"fp32": (PEAK_F32_MFMA_TF, "exact-fp32 MFMA"),
                 "x6": (PEAK_BF16_MFMA_TF / 6, "bf16 MFMA, 6 limb products per fp32 product"),
                 "x3": (PEAK_BF16_MFMA_TF / 3, "bf16 MFMA, 3 limb products per fp32 product")}[gemm_mode]
    mf = sum(d.get("mfma_flops", 0.0) for d in ds) / launches
    return dict(base, bound="mfma", achieved=round(tf, 2), peak=round(peak, 1), unit="TFLOP/s", frac=round(tf / peak, 4),
                mfma_util_executed=round(mf / (ms_avg * 1e-3) / 1e12 / PEAK_BF16_MFMA_TF, 4) if mf else None,
                executed_bf16_mfma_flops=int(mf),
                note=f"achieved / frac: dense-formulation fp32-equivalent flops per launch / HIP-event launch time (comparable with "
                     f"the reference's dense einsum); engine: {eng}; the kernel skips the structurally-zero l<m tiles, so "
                     f"mfma_util_executed = bf16 MFMA flops actually issued (limb products and tile padding included) / time / "
                     f"{PEAK_BF16_MFMA_TF:.0f} TF is the matrix-pipe utilisation (SURVEY.md §8d)")


def load_pmc_traffic(fcn3=False):
    """HBM bytes per launch of every kernel family from the committed PMC passes of THIS command (rocprofv3 counters
    cannot be collected from inside the timed run; the file says how they were taken, tools/pmc_traffic.py rebuilds it — to be
    regenerated whenever a kernel of the family changes).  ONE file, the current round's: a missing file reports no traffic
    (null) rather than an older round's numbers."""
    name = PMC_TRAFFIC_FCN3 if fcn3 else PMC_TRAFFIC
    try:
        with open(os.path.join(ROOT, "profiles", name)) as fh:
            return {k: v["hbm_bytes"] for k, v in json.load(fh).items() if isinstance(v, dict) and "hbm_bytes" in v}
    except (OSError, ValueError):
        return {}


def live_pmc_traffic(cfg_name, timeout_s=None, spectral="train"):
    """HBM bytes per launch of every kernel family, measured IN THIS RUN: two child runs of this same script (the same workload,
    2 eager steps) under ``rocprofv3 --pmc FETCH_SIZE`` and ``--pmc WRITE_SIZE`` — separate passes, counters only, as
    /opt/skills/guides/MI355X_MICROARCH.md prescribes —, summarised per kernel symbol (tools/pmc_summary.py) and mapped to the
    launch families with the guide's gfx950 corrections (tools/pmc_traffic.py).  Returns ({family: bytes}, note); an empty dict
    when rocprofv3 is missing, a pass fails or runs out of time (the caller then falls back to the committed file and says so)."""
    import shutil
    import subprocess
    import tempfile
    if timeout_s is None:
        timeout_s = 420 if CONFIGS.get(cfg_name, {}).get("kind") == "fcn3" else 240
    if shutil.which("rocprofv3") is None:
        return {}, "rocprofv3 not on PATH"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pmc_summary
        import pmc_traffic
    except Exception as e:
        return {}, f"tools/pmc_*.py not importable ({type(e).__name__})"
    work = tempfile.mkdtemp(prefix="mk_pmc_")
    mds = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(work, counter)
            cmd = ["rocprofv3", "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
                   "--config", cfg_name, "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-sht-metric", "--graph", "off", "--no-pmc", "--no-exact",
                   "--spectral", spectral]
            try:
                r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, cwd="/tmp",
                                   env=dict(os.environ, TMPDIR="/tmp"))
            except subprocess.TimeoutExpired:
                return {}, f"the {counter} pass did not finish within {timeout_s} s"
            files = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith("counter_collection.csv")]
            if r.returncode != 0 or not files:
                return {}, f"the {counter} pass failed (rocprofv3 exit code {r.returncode}, {len(files)} counter files)"
            md = os.path.join(work, counter + ".md")
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                pmc_summary.main(md, files)
            mds[counter] = md
        js = os.path.join(work, "traffic.json")
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            pmc_traffic.main(mds["FETCH_SIZE"], mds["WRITE_SIZE"], js, "fcn3" if CONFIGS.get(cfg_name, {}).get("kind") == "fcn3" else "sfno")
        with open(js) as fh:
            data = json.load(fh)
        keep = os.environ.get("MAKANI_AMD_PMC_KEEP")          # tools/profile_round.sh: keep the per-kernel counter tables of this run
        if keep:
            os.makedirs(keep, exist_ok=True)
            for src in (mds["FETCH_SIZE"], mds["WRITE_SIZE"], js):
                shutil.copy(src, os.path.join(keep, os.path.basename(src)))
        return ({k: v["hbm_bytes"] for k, v in data.items() if isinstance(v, dict) and "hbm_bytes" in v},
                "measured in this run: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) over 2 eager steps of the same workload")
    except Exception as e:                       # never lose the benchmark line to the counters
        return {}, f"{type(e).__name__}: {str(e)[:160]}"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def parse_parallelism(par):
    """'dp' -> (1, 1); 'hHwW' -> (H, W)"""
    if par == "dp":
        return 1, 1
    import re
    mt = re.fullmatch(r"h(\d+)w(\d+)", par)
    if not mt:
        raise SystemExit(f"--parallelism {par!r}: expected 'dp' or 'hHwW'")
    return int(mt.group(1)), int(mt.group(2))


def build_model(cfg_name, device, seed):
    import makani_amd as ma
    torch.manual_seed(seed)
    cfg = CONFIGS[cfg_name]
    if cfg.get("kind") == "fcn3":
        return ma.AtmoSphericNeuralOperatorNet(**cfg["model"]).to(device)
    return ma.SphericalFourierNeuralOperatorNet(**cfg).to(device)


def make_optimizer(model, lr=1e-3):
    # AdamW, betas (0.9, 0.95), lr 1e-3, weight decay 0 (config/sfnonet.yaml:50-54,114-117; FourCastNet3: lr 4e-4,
    # config/fourcastnet3.yaml:254-262) as one fused HIP pass per tensor; complex64 spectral weights through their real view.
    from makani_amd.optim import FusedAdamW
    params = [p for p in model.parameters() if p.requires_grad]
    return FusedAdamW(params, lr=lr, betas=(0.9, 0.95), weight_decay=0.0)


def make_ensemble_loss(H, W, channels, device, spatial):
    """FourCastNet3's second-stage loss (config/fourcastnet3.yaml:180-193): "ensemble_crps" (fair CRPS, crps_type
    "skillspread") + 0.1 x "ensemble_spectral_crps", uniform channel weights, mean over (B, C); both on the HIP path
    (makani_amd.CRPSLoss / SpectralCRPSLoss: csrc/crps.hip, the HIP SHT).  pred: (E, C, H, W) — the ensemble members are the
    model's batch —, tar: (1, C, H, W)."""
    import makani_amd as ma
    kw = dict(img_shape=(H, W), crop_shape=(H, W), crop_offset=(0, 0), channel_names=[f"c{i}" for i in range(channels)],
              grid_type="equiangular", crps_type="skillspread", spatial_distributed=spatial)
    crps, scrps = ma.CRPSLoss(**kw).to(device), ma.SpectralCRPSLoss(**kw).to(device)

    def loss(pred, tar):
        f = pred.float().unsqueeze(0)
        return (crps(f, tar) + 0.1 * scrps(f, tar)).mean()
    return loss


def train_step(model, opt, inp, tar, loss_fn, amp, sharded_clip):
    """forward + backward (gradient reductions complete inside backward(): makani_amd.distributed.GradReducer) +
    global-norm clipping + AdamW"""
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        pred = model(inp)
    loss = loss_fn(pred, tar)
    loss.backward()
    if sharded_clip:           # spectral weights sharded over h: their squared norms are summed over that group
        import makani_amd.distributed as thd
        opt.step(grad_scale=thd.clip_coefficient(model, 32.0))
    else:
        opt.step(max_grad_norm=32.0)      # global-norm clipping folded into the AdamW pass
    return loss


DUMP_SEED = 20261016
DUMP_MAX_ELEMENTS = 1 << 22          # per file: 16 MB of float32 for the parameters, as much for the gradients


def _dump_sample(tensors, gen):
    """every tensor flattened (complex through its real view), in order; a tensor larger than its share of
    DUMP_MAX_ELEMENTS contributes that many entries at seeded positions (the same positions in every run)"""
    cap = max(1, DUMP_MAX_ELEMENTS // max(1, len(tensors)))
    parts = []
    for t in tensors:
        flat = (torch.view_as_real(t) if t.is_complex() else t).detach().reshape(-1)
        if flat.numel() > cap:
            idx = torch.randint(flat.numel(), (cap,), generator=gen).sort().values
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    return torch.cat(parts).numpy() if parts else torch.zeros(0).numpy()


def dump_outputs(path, loss, model):
    """--dump-outputs: what the last timed train step handed back, for comparing two builds output for output — its loss,
    and every parameter after the AdamW update with its gradient (named_parameters order; a parameter without a gradient
    contributes zeros)"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    params = [p for _, p in model.named_parameters()]
    grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    np.save(os.path.join(path, "loss.npy"), np.asarray([float(loss.detach().float().reshape(-1)[0])], dtype=np.float64))
    np.save(os.path.join(path, "params.npy"), _dump_sample(params, torch.Generator().manual_seed(DUMP_SEED)))
    np.save(os.path.join(path, "grads.npy"), _dump_sample(grads, torch.Generator().manual_seed(DUMP_SEED)))


def sht_bandwidth(device, reps=5):
    """Secondary metric 'fwd SHT GB/s' (BASELINE.md §2): S1 ERA5-shaped, S2 model-shaped."""
    import makani_amd as ma
    from makani_amd import ops
    out = {}
    for name, C, lmax, mmax in (("S1_c73_L721_M721", 73, 721, 721), ("S2_c384_L240_M241", 384, 240, 241)):
        S = ma.RealSHT(721, 1440, lmax=lmax, mmax=mmax, grid="equiangular").to(device)
        x = torch.rand(1, C, 721, 1440, device=device)
        S(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            S(x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        nbytes = C * 721 * 1440 * 4 + C * lmax * mmax * 8
        out[name] = dict(ms=dt * 1e3, GBps=nbytes / dt / 1e9, spectral_arithmetic=ops.gemm_mode())
        del S, x
        torch.cuda.empty_cache()
    return out


# forward GFLOP per stage of sfno_sc3_layers8_edim384 at 721x1440 (BASELINE.md §2 / SURVEY.md Appendix B)
_STAGE_GF = {"mid_block": 42.6 + 68.23 + 135.9 + 34.0, "total": 4517.7}


def _host_cores():
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)


PARITY_SEED = 20260926


def parity_input(cfg):
    """the input of the in-run parity check: U[0, 1) from a seeded CPU generator, identical in the GPU process and in the
    CPU child (DummyLoader-shaped, makani/utils/dataloaders/data_loader_dummy.py:264-277)"""
    gen = torch.Generator().manual_seed(PARITY_SEED)
    return torch.rand(1, cfg["inp_chans"], *cfg["inp_shape"], generator=gen)


def parity_target(cfg):
    """the target of the in-run gradient parity check (seeded like ``parity_input``)"""
    gen = torch.Generator().manual_seed(PARITY_SEED + 1)
    return torch.rand(1, cfg["out_chans"], *cfg["out_shape"], generator=gen)


# gradients compared end to end: the encoder's first weight (the far end of the backward pass), the spectral
# weights of the first and the last block (both resolution changes), the decoder's last weight, plus the loss and the norm of
# ALL gradients
PARITY_GRADS = ("encoder.fwd.0.weight", "blocks.0.filter.filter.weight", "blocks.7.filter.filter.weight", "decoder.fwd.2.weight")


def _grad_record(model, loss):
    """loss, total gradient norm (fp64 over every parameter) and the PARITY_GRADS gradients of a model after backward()"""
    sq = 0.0
    for p in model.parameters():
        if p.grad is not None:
            g = torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad
            sq += float(g.detach().double().square().sum())
    named = dict(model.named_parameters())
    grads = {n: named[n].grad.detach().cpu().clone() for n in PARITY_GRADS if n in named and named[n].grad is not None}
    return dict(loss=float(loss.detach()), grad_norm=math.sqrt(sq), grads=grads)


def _cpu_worker(cfg_name, mode, state_path=None, out_path=None):
    """child process: the oracle (the reference's model code restated over the restated torch-harmonics SHT), fp32, on
    the host cores.  Always: forward and forward+backward of ONE internal-grid block (seconds; also picks the thread
    count).  mode "step" (default): one full train step (forward + backward + clip + AdamW) of the whole network at
    721 x 1440 (about a minute on the GPU box's host); mode "fwd": its forward pass only.
    ``state_path`` / ``out_path``: the timed forward pass runs with the GPU model's initial weights on ``parity_input``
    and its output is kept — the same pass is the CPU timing sample AND the oracle side of ``parity_rel_l2``."""
    from oracle import sfno as osf
    from oracle import sht as osht
    cores = _host_cores()
    cfg = CONFIGS[cfg_name]
    H, W = cfg["inp_shape"]
    E, sf = cfg["embed_dim"], cfg["scale_factor"]
    h, w = H // sf, W // sf
    torch.manual_seed(333)
    trans = osht.RealSHT(h, w, lmax=h, mmax=w // 2 + 1, grid="legendre-gauss").float()
    itrans = osht.InverseRealSHT(h, w, lmax=h, mmax=w // 2 + 1, grid="legendre-gauss").float()
    blk = osf.NeuralOperatorBlock(trans, itrans, E, "dhconv", cfg["mlp_ratio"], torch.nn.GELU, False)
    x = torch.rand(1, E, h, w, requires_grad=True)
    # thread count: torch's intra-op pools stop scaling long before a two-socket host is full (and collapse when
    # oversubscribed), so the better of 32 and 64 threads is used, measured on the block
    best = None
    for threads in sorted({min(cores, t) for t in (32, 64)}):
        torch.set_num_threads(threads)
        blk(x).square().mean().backward()                  # warm-up (thread pool, allocator)
        t0 = time.perf_counter()
        with torch.no_grad():
            blk(x)
        t_f = time.perf_counter() - t0
        t0 = time.perf_counter()
        x.grad = None
        blk(x).square().mean().backward()
        t_fb = time.perf_counter() - t0
        if best is None or t_fb < best[0]:
            best = (t_fb, t_f, threads)
    t_fb, t_f, threads = best
    rec = dict(t_mid=t_fb, t_mid_fwd=t_f, threads=threads, cores=cores, h=h, w=w, reps=1)
    print(json.dumps(rec), flush=True)
    del blk, x, trans, itrans
    torch.set_num_threads(threads)
    keys = ("inp_shape", "out_shape", "inp_chans", "out_chans", "scale_factor", "embed_dim", "num_layers", "mlp_ratio",
            "operator_type", "model_grid_type", "sht_grid_type")
    model = osf.SphericalFourierNeuralOperatorNet(**{k: cfg[k] for k in keys if k in cfg})
    inp, tar = torch.rand(1, cfg["inp_chans"], H, W), torch.rand(1, cfg["out_chans"], H, W)
    if state_path:
        model.load_state_dict(torch.load(state_path, map_location="cpu"), strict=True)
        inp, tar = parity_input(cfg), parity_target(cfg)
    yb = None
    if out_path:
        # the reference's own arithmetic under op-by-op bf16 autocast (CPU), same weights and input: the yardstick for the
        # GPU path's bf16 distance from the fp32 result (compared below with the fp32 output of the timed pass)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            yb = model(inp).double()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0)
    opt.zero_grad(set_to_none=True)
    t0 = time.perf_counter()
    if mode == "step":
        y = model(inp)                                         # the forward pass of the train step (graph kept for backward)
    else:
        with torch.no_grad():
            y = model(inp)
    rec.update(t_fwd=time.perf_counter() - t0, out_mean=float(y.detach().mean()))
    t_aux = time.perf_counter()                                # (bookkeeping between forward and backward is not part of the step)
    if out_path:
        torch.save(y.detach(), out_path)
        yd = y.detach().double()
        rec.update(parity_output=out_path, oracle_bf16_rel_l2=float((yb - yd).norm() / yd.norm()))
        del yb, yd
    print(json.dumps(rec), flush=True)                         # from here on the parent has the forward time and the parity output
    if mode != "step":
        return
    t_aux = time.perf_counter() - t_aux
    loss = (y - tar).square().mean()
    loss.backward()
    t_aux2 = time.perf_counter()
    if out_path:                                               # the oracle side of the gradient parity (bookkeeping, not timed)
        torch.save(_grad_record(model, loss), out_path + ".grads")
    t_aux += time.perf_counter() - t_aux2
    torch.nn.utils.clip_grad_norm_(model.parameters(), 32.0)
    opt.step()
    rec.update(t_step=time.perf_counter() - t0 - t_aux, loss=float(loss.detach()))
    print(json.dumps(rec), flush=True)
    if out_path and state_path:
        # after the measurement (a time-out from here on loses nothing of it): the yardstick of the bf16 gradient figures — the
        # oracle's OWN backward pass under op-by-op CPU bf16 autocast on the initial weights, same input / target / loss, as
        # oracle_bf16_rel_l2 is the yardstick of the bf16 forward figure
        del y, loss
        model.load_state_dict(torch.load(state_path, map_location="cpu"), strict=True)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y16 = model(inp)
        l16 = (y16.float() - tar).square().mean()
        l16.backward()
        torch.save(_grad_record(model, l16), out_path + ".grads_bf16")


def fcn3_parity_input(cin, h, w):
    """input of the FourCastNet3 line's in-run block parity: seeded U[0, 1), identical in the GPU process and in the CPU child"""
    return torch.rand(1, cin, h, w, generator=torch.Generator().manual_seed(PARITY_SEED + 2))


def _cpu_worker_fcn3(cfg_name, state_path=None, out_path=None):
    """child process of the FourCastNet3 line: the oracle's processor blocks (oracle/fcn3.py — the reference's network code restated,
    pinned by fixtures written by the reference's own module: tests/test_oracle_fcn3.py) at the REAL internal grid and width, fp32,
    one ensemble member.  Bounded sample: one "global" block (spectral convolution + MLP) and one "local" block (DISCO convolution
    with the doubled cutoff + MLP), each whole, forward and forward + backward; the thread count is the faster of 32 / 64 on the
    global block.  Encoders / decoders (five DISCO convolutions on the 721 x 1440 grid), the CRPS losses and the optimizer are NOT
    in the sample: the figure derived from it is an upper bound of the host's training rate."""
    from oracle import disco as od
    from oracle import fcn3 as ofc
    from oracle import sht as osht
    cores = _host_cores()
    cfg = CONFIGS[cfg_name]
    m = cfg["model"]
    H, W = m["inp_shape"]
    h, w = H // m["scale_factor"], W // m["scale_factor"]
    _, _, _, _, levels = ofc.get_channel_groups(m["channel_names"], m["aux_channel_names"])
    total = len(levels) * m["atmo_embed_dim"] + m["surf_embed_dim"]
    cin = total + m["aux_embed_dim"]
    n_global = len([i for i in range(m["num_layers"]) if i % m["sfno_block_frequency"] == 0])
    n_local = m["num_layers"] - n_global
    torch.manual_seed(333)
    od.DiscreteContinuousConvS2.contraction = "direct"
    grid = m.get("sht_grid_type", "legendre-gauss")
    sht = osht.RealSHT(h, w, lmax=h, mmax=w // 2 + 1, grid=grid).float()
    isht = osht.InverseRealSHT(h, w, lmax=h, mmax=w // 2 + 1, grid=grid).float()
    kw = dict(mlp_ratio=m.get("mlp_ratio", 2.0), normalization_layer=m.get("normalization_layer", "none"), use_mlp=m.get("use_mlp", True),
              kernel_shape=tuple(m["kernel_shape"]), basis_type=m["filter_basis_type"], bias=m.get("bias", False))
    x = (fcn3_parity_input(cin, h, w) if state_path else torch.rand(1, cin, h, w)).requires_grad_(True)
    state = torch.load(state_path, map_location="cpu") if state_path else None
    outputs = {}

    def timed(blk):
        t0 = time.perf_counter()
        with torch.no_grad():
            blk(x)
        t_f = time.perf_counter() - t0
        x.grad = None
        t0 = time.perf_counter()
        blk(x).square().mean().backward()
        return t_f, time.perf_counter() - t0
    blk = ofc.NeuralOperatorBlock(sht, isht, cin, total, conv_type="global", **kw)
    if state is not None:                                      # the GPU model's own blocks: the timed passes are the parity passes
        blk.load_state_dict(state["global"], strict=True)
        with torch.no_grad():
            outputs["global"] = blk(x).detach().clone()
    best = None
    for threads in sorted({min(cores, t) for t in (32, 64)}):
        torch.set_num_threads(threads)
        with torch.no_grad():
            blk(x)                                             # warm-up (thread pool, allocator)
        t_f, t_fb = timed(blk)
        if best is None or t_fb < best[1]:
            best = (t_f, t_fb, threads)
    t_f, t_fb, threads = best
    torch.set_num_threads(threads)
    rec = dict(t_global=t_f, t_global_fb=t_fb, threads=threads, cores=cores, h=h, w=w, channels=cin, n_global=n_global, n_local=n_local,
               members=cfg["ensemble_size"])
    print(json.dumps(rec), flush=True)
    del blk
    blk = ofc.NeuralOperatorBlock(sht, isht, cin, total, conv_type="local", **kw)
    rec["psi_entries"] = int(blk.local_conv.psi_vals.numel())
    if state is not None:
        blk.load_state_dict(state["local"], strict=True)
    t0 = time.perf_counter()
    with torch.no_grad():
        y = blk(x)
    rec["t_local"] = time.perf_counter() - t0
    if state is not None and out_path:
        outputs["local"] = y.detach()
        torch.save(outputs, out_path)
        rec["parity_output"] = out_path
    del y
    print(json.dumps(rec), flush=True)                         # forward-only figures complete from here on
    x.grad = None
    t0 = time.perf_counter()
    blk(x).square().mean().backward()
    rec["t_local_fb"] = time.perf_counter() - t0
    print(json.dumps(rec), flush=True)


class ParityProbe:
    """In-run parity of the measured model against the oracle: before the first train step the
    GPU model — initial weights, ``parity_input`` / ``parity_target`` — runs forward (fp32 and bf16 autocast, the benchmark's
    precision) and forward + backward of ``mean((y - target)^2)`` (fp32 and bf16 autocast); its initial weights go to a scratch
    file.  The CPU child that times the oracle's full train step loads those weights, runs the same input / target / loss and
    keeps its output and its gradients (before clipping); ``finish`` reports the rel-L2 distances of the output, of the loss,
    of the norm of ALL gradients and of the four gradients of ``PARITY_GRADS``."""

    def __init__(self, model, cfg, device):
        import tempfile
        self.dir = tempfile.mkdtemp(prefix="mk_parity_")
        self.oracle_bf16 = None
        self.state_path = os.path.join(self.dir, "state.pt")
        self.out_path = os.path.join(self.dir, "oracle_out.pt")
        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, self.state_path)
        x, tar = parity_input(cfg).to(device), parity_target(cfg).to(device)
        was_training = model.training
        model.eval()
        # the fp32 passes compare with the fp32 oracle at the reference's TEST settings (tests/testutils.py: disable_tf32): exact
        # fp32-class spectral arithmetic; the bf16 autocast passes run as the benchmark does (the process-wide setting)
        tf32_was = torch.backends.cuda.matmul.allow_tf32
        with torch.no_grad():
            torch.backends.cuda.matmul.allow_tf32 = False
            self.y32 = model(x).float().cpu()
            torch.backends.cuda.matmul.allow_tf32 = tf32_was
            with torch.autocast("cuda", dtype=torch.bfloat16):
                self.y16 = model(x).float().cpu()
        model.train(was_training)
        self.bwd = {}
        for name, amp in (("fp32", False), ("bf16_autocast", True)):
            model.zero_grad(set_to_none=True)
            torch.backends.cuda.matmul.allow_tf32 = tf32_was if amp else False
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                y = model(x)
            loss = (y.float() - tar).square().mean()
            loss.backward()
            torch.backends.cuda.matmul.allow_tf32 = tf32_was
            self.bwd[name] = _grad_record(model, loss)
            del y, loss
        model.zero_grad(set_to_none=True)
        del x, tar
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()                       # peak_hbm_GB is the train loop's, not the probe's

    @staticmethod
    def _rel(a, b):
        a = torch.view_as_real(a) if a.is_complex() else a
        b = torch.view_as_real(b) if b.is_complex() else b
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))

    def finish(self):
        import shutil
        out = None
        try:
            if os.path.exists(self.out_path):
                yo = torch.load(self.out_path, map_location="cpu").double()
                den = float(yo.norm())
                out = dict(fp32=float((self.y32.double() - yo).norm()) / den, bf16_autocast=float((self.y16.double() - yo).norm()) / den,
                           oracle_bf16_autocast=self.oracle_bf16,
                           bf16_gate="relative to the oracle's own bf16 autocast (oracle_bf16_autocast), not the flat 2e-2 of BASELINE.md §3",
                           what="rel-L2 of the GPU model's forward output (initial weights of this run, seeded U[0,1) input, "
                                "721x1440x73, all 8 layers) against the fp32 CPU oracle's output of the pass timed as "
                                "cpu_baseline; oracle_bf16_autocast = the same distance for the oracle itself under op-by-op CPU "
                                "bf16 autocast (the reference's own bf16 arithmetic).  Gates: fp32 <= 1e-4 (BASELINE.md §3); bf16 "
                                "autocast <= the oracle's own bf16 distance (2e-2 holds per block, not through 8 bf16 layers).  "
                                "grad_*: the same run's backward pass of mean((y - target)^2) against the oracle's backward pass "
                                "(the one timed inside cpu_baseline's train step): loss, norm of all gradients (relative "
                                "difference) and rel-L2 of four gradients; gate fp32 <= 1e-4; every *_bf16 figure sits beside oracle_bf16_grad_* = "
                                "the same distance for the oracle's own backward pass under CPU bf16 autocast (gate: <= 1.25 x that, "
                                "tests/test_gpu_headline.py)")
            gpath = self.out_path + ".grads"
            if out is not None and os.path.exists(gpath + "_bf16") and os.path.exists(gpath):
                # oracle_bf16_grad_*: how far the reference's own bf16 arithmetic (CPU autocast) moves each of these quantities
                # from its fp32 value — the yardstick every grad_*_bf16 figure below sits beside
                ref, r16 = torch.load(gpath, map_location="cpu"), torch.load(gpath + "_bf16", map_location="cpu")
                out["oracle_bf16_grad_loss"] = abs(r16["loss"] - ref["loss"]) / abs(ref["loss"])
                out["oracle_bf16_grad_norm"] = abs(r16["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"]
                for n, g in r16["grads"].items():
                    if n in ref["grads"]:
                        out[f"oracle_bf16_grad_{n}"] = self._rel(g, ref["grads"][n])
            if out is not None and os.path.exists(gpath):
                ref = torch.load(gpath, map_location="cpu")
                for name, rec in self.bwd.items():
                    sfx = "" if name == "fp32" else "_bf16"
                    out[f"grad_loss{sfx}"] = abs(rec["loss"] - ref["loss"]) / abs(ref["loss"])
                    out[f"grad_norm{sfx}"] = abs(rec["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"]
                    for n, g in rec["grads"].items():
                        if n in ref["grads"]:
                            out[f"grad_{n}{sfx}"] = self._rel(g, ref["grads"][n])
        finally:
            shutil.rmtree(self.dir, ignore_errors=True)
        return out


class Fcn3ParityProbe:
    """In-run parity of the FourCastNet3 line, block level: the first "global" and the first "local" processor block of the measured
    model — its initial weights, a seeded input of the real internal shape — run forward on the GPU in fp32 and under bf16 autocast;
    their weights go to a scratch file.  The CPU child that times the oracle's blocks loads those weights and runs the same input:
    its timed forward passes ARE the oracle side of ``parity_rel_l2``.  (The whole network's forward pass is many minutes of host
    time; the whole network is compared against fixtures of the reference's own module in tests/test_fcn3.py.)"""

    def __init__(self, model, cfg, device):
        import tempfile
        self.dir = tempfile.mkdtemp(prefix="mk_parity_fcn3_")
        self.state_path = os.path.join(self.dir, "blocks.pt")
        self.out_path = os.path.join(self.dir, "oracle_blocks.pt")
        self.oracle_bf16 = None
        blocks = {"global": next(b for b in model.blocks if hasattr(b, "global_conv")),
                  "local": next(b for b in model.blocks if hasattr(b, "local_conv"))}
        torch.save({k: {n: v.detach().cpu() for n, v in b.state_dict().items()} for k, b in blocks.items()}, self.state_path)
        h, w = blocks["global"].inp_shape
        cin = model.total_embed_dim + (model.aux_embed_dim if model.n_aux_chans > 0 else 0)
        x = fcn3_parity_input(cin, h, w).to(device)
        self.y32, self.y16 = {}, {}
        with torch.no_grad():
            for k, b in blocks.items():
                self.y32[k] = b(x).float().cpu()
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    self.y16[k] = b(x).float().cpu()
        del x
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    def finish(self):
        import shutil
        out = None
        try:
            if os.path.exists(self.out_path):
                ref = torch.load(self.out_path, map_location="cpu")
                out = {}
                for k in ("global", "local"):
                    if k in ref:
                        yo = ref[k].double()
                        out[f"{k}_block_fp32"] = float((self.y32[k].double() - yo).norm() / yo.norm())
                        out[f"{k}_block_bf16_autocast"] = float((self.y16[k].double() - yo).norm() / yo.norm())
                out["what"] = ("rel-L2 of the forward output of the measured model's first global (spectral convolution + MLP) and first local "
                               "(DISCO convolution + MLP) processor block — initial weights of this run, seeded U[0,1) input of the real internal "
                               "shape — against the fp32 CPU oracle's output of the passes timed as cpu_baseline.  Gates: fp32 <= 1e-4 "
                               "(BASELINE.md §3, end to end), bf16 autocast <= 2e-2 per block")
        finally:
            shutil.rmtree(self.dir, ignore_errors=True)
        return out


def cpu_baseline(cfg_name, timeout_s=420, parity=None):
    """Reference-equivalent CPU path, timed in a child process on this host's cores, fp32 (kind "port": the oracle — the
    reference's own modules cannot be imported on the benchmark host, /root/reference exists in the build container only; the
    oracle restates them and is pinned by fixtures generated from them).  Bounded sample: ONE full train step (forward +
    backward + clip + AdamW) of the whole network at 721 x 1440, B = 1 (about 60 s on 32 threads of the GPU box's host;
    round 3 — round 2 reported forward x block ratio because an earlier attempt had not finished).  Fallbacks, taken from the
    records the child prints as it goes, when the step does not finish inside the time limit (or MAKANI_AMD_CPU_BASELINE=fwd):
    the measured forward pass times the (forward+backward)/forward ratio measured on one internal-grid block; then the block
    alone scaled by the step/block FLOP ratio.  ``sample`` says which one was reported."""
    import subprocess
    if CONFIGS.get(cfg_name, {}).get("kind") == "fcn3":
        return cpu_baseline_fcn3(cfg_name, timeout_s, parity)
    if cfg_name != "sfno_sc3_layers8_edim384":
        return None
    mode = os.environ.get("MAKANI_AMD_CPU_BASELINE", "step")
    recs, err = [], None
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", cfg_name, "--cpu-mode", mode]
        if parity is not None:
            cmd += ["--cpu-state", parity.state_path, "--cpu-out", parity.out_path]
        pr = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        try:
            so, _ = pr.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            pr.kill()
            so, _ = pr.communicate()
            err = f"time limit {timeout_s} s"
        recs = [json.loads(l) for l in (so or "").splitlines() if l.startswith("{")]
        if pr.returncode not in (0, None) and err is None:
            err = f"exit code {pr.returncode}"
    except Exception as e:   # never stall the GPU benchmark
        err = type(e).__name__
    if not recs:
        return dict(value=None, unit="samples/s", cores=None, kind="port", sample=f"CPU baseline unavailable: {err}")
    rec = recs[-1]
    if parity is not None:
        parity.oracle_bf16 = rec.get("oracle_bf16_rel_l2")
    who = f"oracle fp32 on {rec['threads']} host threads ({rec['cores']} cores visible; the faster of 32 / 64 threads on one block)"
    if "t_step" in rec:
        return dict(value=1.0 / rec["t_step"], unit="samples/s", cores=rec["threads"], kind="port",
                    sample=f"{who}: ONE measured full train step (fwd + bwd + clip + AdamW) of the whole network at 721x1440, "
                           f"B=1 = {rec['t_step']:.1f} s (its forward pass: {rec['t_fwd']:.1f} s)",
                    ms_per_step=rec["t_step"] * 1e3, measured="full step")
    if "t_fwd" in rec:
        ratio = rec["t_mid"] / rec["t_mid_fwd"]
        step = rec["t_fwd"] * ratio
        return dict(value=1.0 / step, unit="samples/s", cores=rec["threads"], kind="port",
                    sample=f"{who}: ONE measured forward pass of the whole network at 721x1440, B=1 = {rec['t_fwd']:.1f} s, times the "
                           f"measured (fwd+bwd)/fwd ratio of one internal-grid block ({rec['t_mid']:.2f} s / {rec['t_mid_fwd']:.2f} s = "
                           f"{ratio:.2f}) -> {step:.1f} s per step; optimizer excluded"
                           + (f" (the full step did not finish: {err})" if (mode == "step" and err) else ""),
                    ms_per_step=step * 1e3, measured="full-size forward x block bwd/fwd ratio")
    scale = _STAGE_GF["total"] / _STAGE_GF["mid_block"]
    step = rec["t_mid"] * scale
    return dict(value=1.0 / step, unit="samples/s", cores=rec["threads"], kind="port",
                sample=f"{who}: the whole-network pass did not complete ({err}); fwd+bwd of one internal-grid block "
                       f"({rec['h']}x{rec['w']}, 384 ch) = {rec['t_mid']:.2f} s, scaled by the step/block FLOP ratio {scale:.1f} -> "
                       f"{step:.1f} s per step (optimizer excluded)",
                ms_per_step=step * 1e3, measured="one block, extrapolated")


def cpu_baseline_fcn3(cfg_name, timeout_s=420, parity=None):
    """``cpu_baseline`` of the FourCastNet3 line: see ``_cpu_worker_fcn3`` for the sample (processor blocks only)."""
    import subprocess
    recs, err = [], None
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", cfg_name]
        if parity is not None:
            cmd += ["--cpu-state", parity.state_path, "--cpu-out", parity.out_path]
        pr = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        try:
            so, _ = pr.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            pr.kill()
            so, _ = pr.communicate()
            err = f"time limit {timeout_s} s"
        recs = [json.loads(l) for l in (so or "").splitlines() if l.startswith("{")]
        if pr.returncode not in (0, None) and err is None:
            err = f"exit code {pr.returncode}"
    except Exception as e:   # never stall the GPU benchmark
        err = type(e).__name__
    if not recs or "t_local" not in recs[-1]:
        return dict(value=None, unit="samples/s", cores=None, kind="port", sample=f"CPU baseline unavailable: {err}")
    r = recs[-1]
    fb = "t_local_fb" in r
    t_g, t_l = (r["t_global_fb"], r["t_local_fb"]) if fb else (r["t_global"], r["t_local"])
    t_sample = r["members"] * (r["n_global"] * t_g + r["n_local"] * t_l)
    what = "forward + backward" if fb else "FORWARD ONLY (the backward sample did not finish: " + str(err) + ")"
    return dict(value=1.0 / t_sample, unit="samples/s", cores=r["threads"], kind="port", measured=f"processor blocks, {'fwd + bwd' if fb else 'fwd only'}",
                ms_per_step=t_sample * 1e3,
                sample=(f"oracle fp32 (oracle/fcn3.py) on {r['threads']} host threads ({r['cores']} cores visible), PROCESSOR BLOCKS ONLY, {what}, at the "
                        f"real internal grid {r['h']}x{r['w']} and width {r['channels']}: one global block (spectral convolution + MLP) = "
                        f"{t_g:.1f} s (its forward pass {r['t_global']:.1f} s), one local block (DISCO convolution, {r['psi_entries']} entries of psi "
                        f"per output longitude, + MLP) = {t_l:.1f} s (forward {r['t_local']:.1f} s); x ({r['n_global']} global + {r['n_local']} local "
                        f"blocks) x {r['members']} ensemble members = {t_sample:.0f} s per sample.  The encoders / decoders (DISCO convolutions "
                        f"on the 721x1440 grid), the CRPS losses and the optimizer are NOT included: an UPPER bound of the host's training "
                        f"rate, not a measured train step"))


def default_parallelism(world, cfg_name="sfno_sc3_layers8_edim384"):
    """the north-star split over ALL GPUs of the node (BASELINE.json: h_parallel=4, w_parallel=2 at 8 GPUs); FourCastNet3
    (configs[3]): "8 MI355X, h=2 w=2 + data-parallel" """
    if CONFIGS.get(cfg_name, {}).get("kind") == "fcn3":
        return {1: "dp", 2: "h2w1", 4: "h2w2", 8: "h2w2"}.get(world, "dp")
    # 2 GPUs: data parallel.  BASELINE.json prescribes the spatial split for 4 (configs[2]: h = 4) and 8 GPUs (configs[4]: h4 w2)
    # only; the reference's partitioning has no 2-GPU split worth running on xGMI — h2 w1 sends 3.7 GB per step and rank over the
    # ONE link between the two GPUs (24 ms at 153 GB/s: slower than one GPU, profiles/r05_shard_shapes.md) — while two
    # data-parallel replicas exchange 2.3 GB of gradients behind their backward passes.  `--parallelism h2w1` still runs it.
    return {1: "dp", 2: "dp", 4: "h4w1", 8: "h4w2"}.get(world, "dp")


def run_worker(args):
    """one rank of the measurement; rank 0 returns the result dict, the others None"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("MAKANI_AMD_BENCH_BACKEND", "nccl")    # "gloo": functional test of N ranks on one GPU
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        import datetime
        to = datetime.timedelta(seconds=int(os.environ.get("MAKANI_AMD_BENCH_PG_TIMEOUT", "150")))
        if backend == "nccl" and os.environ.get("MAKANI_AMD_BENCH_GRAPH", args.graph) != "off":
            # the captured step (below) contains RCCL send / recv collectives; torch 2.10's process group hands their work to its
            # watchdog thread, whose event query then fails ("operation not permitted on an event last recorded in a capturing
            # stream") and would take the process down.  With these settings the watchdog thread just ends at that point
            # (tests/test_gpu_distributed.py::test_hipgraph_capture_of_the_distributed_blocks_with_rccl_world1)
            os.environ.setdefault("TORCH_NCCL_RETHROW_CUDA_ERRORS", "0")
            os.environ.setdefault("TORCH_NCCL_ENABLE_MONITORING", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device, timeout=to)
        else:
            dist.init_process_group(backend, timeout=to)

    from makani_amd import ops
    import makani_amd.comm as mcomm
    import makani_amd.distributed as thd

    # ---- process-group tree: world -> data x (h x w), as makani/utils/comm.py:114-201 ----
    par = args.parallelism if args.parallelism != "auto" else default_parallelism(world, args.config)
    ph, pw = parse_parallelism(par)
    msize = ph * pw
    if world % msize:
        raise SystemExit(f"world size {world} is not a multiple of h*w = {msize}")
    dsize = world // msize
    d_idx, ih, iw = mcomm.init(ph, pw)      # the network initialises the transform layer from this tree (sfnonet.py:786-789)

    cfg = CONFIGS[args.config]
    H, W = cfg["inp_shape"]
    B = 1
    fcn3 = cfg.get("kind") == "fcn3"
    E = cfg["ensemble_size"] if fcn3 else 1                        # ensemble members ride in the model's batch dimension
    if fcn3 and args.multistep_count > 1:
        raise SystemExit("--multistep-count applies to the SFNO workloads")
    model = build_model(args.config, device, seed=333)            # same seed on every rank -> same init
    opt = make_optimizer(model, lr=cfg.get("lr", 1e-3))
    probe = None
    if world == 1 and args.full and not args.no_cpu_baseline and args.config == "sfno_sc3_layers8_edim384":
        probe = ParityProbe(model, cfg, device)                    # before the first update: the weights the oracle will load
    elif world == 1 and args.full and not args.no_cpu_baseline and fcn3:
        try:
            probe = Fcn3ParityProbe(model, cfg, device)            # block level (the whole network is minutes of host time)
        except Exception as e:                                     # the probe must never cost the measurement
            print(f"[bench] FourCastNet3 parity probe unavailable: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
    # mappings.py:321-525 (the model itself when world == 1); --zero: ZeRO-1 over the data group (reduce-scattered
    # gradients, sharded AdamW state, in-place parameter all-gather: makani_amd/optim.py)
    net = thd.init_gradient_reduction_hooks(model, device, zero=args.zero and dsize > 1)
    if args.multistep_count > 1:                                   # makani/models/stepper.py:176-345
        from makani_amd.stepper import MultiStepWrapper
        net = MultiStepWrapper(net, n_future=args.multistep_count - 1, multistep_checkpoint=args.multistep_checkpoint).train()
    torch.manual_seed(333 + d_idx)                                 # DummyLoader: fixed U[0,1) tensors on device
    inp = torch.rand(B * E, cfg["inp_chans"], H, W, device=device)
    if fcn3:
        # one initial condition per sample: the state and static channels are shared by the members, the noise channels are
        # drawn per member (fixed synthetic draws, resident like the rest of the input; makani samples them per step from a
        # spherical diffusion process in its preprocessor, outside this path)
        names = cfg["model"]["channel_names"] + cfg["model"]["aux_channel_names"]
        shared = [i for i, n in enumerate(names) if not n.startswith("xnoise")]
        inp[:, shared] = inp[:1, shared]
        noise = [i for i, n in enumerate(names) if n.startswith("xnoise")]
        inp[:, noise] = torch.randn(B * E, len(noise), H, W, device=device)
    tar = torch.rand(B, cfg["out_chans"] * args.multistep_count, H, W, device=device)
    if fcn3:
        loss_fn = make_ensemble_loss(H, W, cfg["out_chans"], device, msize > 1)
    else:
        loss_fn = make_loss(H, W, cfg["out_chans"] * args.multistep_count, device, msize > 1)
    if msize > 1:                                                  # this rank's lat/lon shard (dataloaders shard likewise)
        lats, lons = thd.compute_split_shapes(H, ph), thd.compute_split_shapes(W, pw)
        lat0, lon0, hl, wl = sum(lats[:ih]), sum(lons[:iw]), lats[ih], lons[iw]
        inp = inp[..., lat0:lat0 + hl, lon0:lon0 + wl].contiguous()
        tar = tar[..., lat0:lat0 + hl, lon0:lon0 + wl].contiguous()
    amp = not args.fp32
    sharded_clip = ph > 1
    # fp32 matrix products as the reference's TRAINING entry points run them: makani/train.py:87-88 (train_stochastic.py:102-103)
    # set torch.backends.cuda.matmul.allow_tf32 = True, so on the reference's GPUs the fp32 einsums of the SHT and of the spectral
    # contraction run in TF32 (10 mantissa bits).  gfx950 has no TF32 mode; makani_amd reads the same torch switch and then runs
    # its spectral GEMMs on TWO bf16 limbs per fp32 factor (3 limb products, rel-L2 ~4e-6 vs fp64: 64x closer than TF32) instead
    # of three (6 products, 1.8e-7).  --spectral exact leaves torch's default (and the reference's TEST setting) in place; the
    # default run measures that variant too and reports it as `exact_fp32_spectral`.
    spectral_train = amp and args.spectral == "train"
    torch.backends.cuda.matmul.allow_tf32 = bool(spectral_train)

    # Per-kernel HIP events cost ~1.2 ms/step (2 events x ~300 C-ABI launches), so only --full records them.  The LAST
    # warm-up step is profiled in full: it yields the per-kernel table and names the dominant HIP kernel; inside the timed
    # region only that kernel carries events (its roofline numbers therefore come from the timed steps).  With
    # --warmup 0 every launch of the timed region is instrumented instead.
    # Python's cyclic collector is paused for the warm-up and the timed loop: a generation-2 collection over the
    # autograd graphs stalls the launching thread for ~100 ms (measured with tools/step_times.py: one step of 154 ms
    # among 54 ms steps), enough to drain the GPU queue.  Reference counting still frees every tensor immediately.
    import gc
    gc.collect()
    gc.disable()
    warm_prof, dom_family, dom_members = {}, None, []
    for i in range(args.warmup):
        last = args.full and i == args.warmup - 1
        if last:
            torch.cuda.synchronize()
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
        train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
        if last:
            torch.cuda.synchronize()
            ops.PROFILER.enabled = False
            warm_prof = ops.PROFILER.summary()
            dom_family, dom_members = dominant_family(warm_prof)
    torch.cuda.synchronize()

    # ---- hipGraph: the whole step (forward, backward, clip, AdamW: ~380 dependent launches) captured once, replayed
    # per step.  Nothing in the step depends on host state (the optimizer's step counter lives in device memory,
    # inputs are static tensors, the distributed norm's shard counts stay on the device), so a replay IS the step.
    # N > 1 over RCCL: the collectives are captured WITH the step (RCCL's kernels are ordinary stream work; torch's process
    # group records them on the capturing streams).  It is what makes the h x w step scale at all: eager, one rank of h4 w2
    # launches for 34 ms per step while its kernels run for 11 (tools/shadow_rank.py, profiles/r05_shard_shapes.md).  Every
    # rank must take the same path — a rank replaying a graph and a rank launching eagerly would still match collective by
    # collective, but a rank whose capture failed half-way would not —, so the ranks agree on the outcome before the first
    # replay; MAKANI_AMD_BENCH_GRAPH=off (set by the launcher's retry) forces the eager step.  gloo (N ranks on one GPU) is
    # host-staged and cannot be captured.
    graph, graph_note = None, None
    graph_mode = os.environ.get("MAKANI_AMD_BENCH_GRAPH", args.graph)
    want_graph = graph_mode == "on" or (graph_mode == "auto" and (world == 1 or backend == "nccl"))
    if world > 1 and CONFIGS[args.config].get("kind") == "fcn3" and graph_mode != "on":
        want_graph = False          # the DISCO halo exchange is a batched isend / irecv, which does not survive capture here
    capture_tried = want_graph and world > 1              # (decides the teardown at the end of this function)
    if want_graph:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                     # one eager step on a side stream (torch's capture recipe)
                eager_loss = train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            opt.zero_grad(set_to_none=True)
            graph = torch.cuda.CUDAGraph()
            # N > 1: "thread_local" — the process group's watchdog thread polls events while this thread captures
            with torch.cuda.graph(graph, capture_error_mode="global" if world == 1 else "thread_local"):
                graph_loss = train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
            torch.cuda.synchronize()
        except Exception as e:                                # capture is an optimisation: never lose the measurement to it
            graph, graph_note = None, f"graph capture failed ({type(e).__name__}: {str(e)[:200]}); eager launches"
            print(f"[bench] {graph_note}", file=sys.stderr, flush=True)
            torch.cuda.synchronize()
        if world > 1:                                         # all ranks replay, or none does
            flag = torch.tensor([1 if graph is not None else 0], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0 and graph is not None:
                graph, graph_note = None, "another rank's graph capture failed; eager launches on every rank"
        if graph is not None:
            graph.replay()                                    # first replay outside the timed region
            torch.cuda.synchronize()
            # a replay whose loss is not a finite number (a collective that did not survive the capture) must not be timed: every
            # rank checks its own replayed loss, the ranks agree, and on disagreement all fall back to eager launches
            # ... and it must be the loss of THIS training run: one optimizer update away from the eager step just before the capture
            # (same data: within a factor of two of it), not the residue of a collective that replays differently than it captured
            gl, el = graph_loss.detach().float().reshape(-1)[0], eager_loss.detach().float().reshape(-1)[0]
            okf = (torch.isfinite(gl) & ((gl - el).abs() <= 0.5 * el.abs() + 1e-12)).to(torch.int32).reshape(1)
            if world > 1:
                dist.all_reduce(okf, op=dist.ReduceOp.MIN)
            if int(okf.item()) == 0:
                graph, graph_note = None, "the first replay of the captured step produced a loss that is not finite or far from the eager step's; eager launches"
                print(f"[bench] {graph_note}", file=sys.stderr, flush=True)

    ops.PROFILER.reset()
    ops.PROFILER.enabled = args.full and graph is None
    ops.PROFILER.only = set(dom_members) if dom_members else None      # HIP events on the dominant kernel only (see above)
    thd.COMM_STATS.clear()                                             # all-to-all accounting of the timed steps (N > 1)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if graph is not None:
        for _ in range(args.steps):
            graph.replay()
        loss = graph_loss
    else:
        for _ in range(args.steps):
            loss = train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
    torch.cuda.synchronize()
    gc.enable()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ops.PROFILER.enabled = False
    if args.dump_outputs and rank == 0:          # before anything below runs another step on the same weights
        dump_outputs(args.dump_outputs, loss, model)
    comm_stats = {f"{k[0]}_group_of_{k[1]}": dict(MB_sent=round(v["bytes_sent"] / args.steps / 1e6, 2), all_to_alls=v["all_to_alls"] / args.steps)
                  for k, v in sorted(thd.COMM_STATS.items())}
    event_steps = args.steps
    if graph is not None and args.full:
        # launch durations of the dominant kernel: HIP events cannot bracket a node inside a replayed graph, so the same
        # launches are timed in eager steps right after the timed region (same process, same tensors, same shapes)
        event_steps = 3
        ops.PROFILER.reset()
        ops.PROFILER.enabled = True
        thd.COMM_STATS.clear()                  # (a replayed graph does not pass through the Python accounting of the exchanges)
        for _ in range(event_steps):
            train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
        torch.cuda.synchronize()
        ops.PROFILER.enabled = False
        comm_stats = {f"{k[0]}_group_of_{k[1]}": dict(MB_sent=round(v["bytes_sent"] / event_steps / 1e6, 2), all_to_alls=v["all_to_alls"] / event_steps)
                      for k, v in sorted(thd.COMM_STATS.items())}

    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()
    # the same step with the spectral GEMMs in fp32-class arithmetic (three limbs): captured and timed the same way, reported
    # beside the headline so that both settings of the switch are on record from ONE run
    exact = None
    if args.full and spectral_train and world == 1 and graph is not None and not args.no_exact:
        try:
            torch.backends.cuda.matmul.allow_tf32 = False
            for _ in range(2):
                train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
            torch.cuda.synchronize()
            opt.zero_grad(set_to_none=True)
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                train_step(net, opt, inp, tar, loss_fn, amp, sharded_clip)
            g2.replay()
            torch.cuda.synchronize()
            t0x = time.perf_counter()
            for _ in range(args.steps):
                g2.replay()
            torch.cuda.synchronize()
            ex = time.perf_counter() - t0x
            exact = {"value": dsize * B * args.steps / ex, "unit": "samples/s", "ms_per_step": ex / args.steps * 1e3,
                     "spectral_arithmetic": "three bf16 limbs per fp32 factor, 6 limb products: rel-L2 1.8e-7 vs fp64 (torch's default "
                                            "allow_tf32 = False; what the reference's tests set)"}
            del g2
        except Exception as e:
            exact = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
        finally:
            torch.backends.cuda.matmul.allow_tf32 = True
    final_loss = float(loss.detach())

    out = None
    if rank == 0:
        out = {
            "metric": (f"FourCastNet3 train samples/sec at {H}x{W}x{cfg['out_chans']}ch" if fcn3 else
                       f"SFNO train samples/sec at {H}x{W}x{cfg['inp_chans']}ch"),
            "value": dsize * B * args.steps / elapsed,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak" if msize == 1 else ("strong" if dsize == 1 else "mixed"),
            "vs_baseline": None,
            "dtype": "bf16" if amp else "f32",
            "data": "synthetic",
            "config": {"workload": args.config, "grid": f"{H}x{W}", "channels": cfg["inp_chans"],
                       **({"ensemble_size": E, "loss": "ensemble_crps (skillspread) + 0.1 x ensemble_spectral_crps",
                           "state_channels": cfg["out_chans"], "aux_channels": cfg["inp_chans"] - cfg["out_chans"]} if fcn3 else {}),
                       "global_batch": dsize * B, "parallelism": f"dp{dsize}" + (f"_h{ph}w{pw}" if msize > 1 else ""),
                       "amp": ("bf16 autocast, fp32 SHT/contraction" + (" under torch.backends.cuda.matmul.allow_tf32 = True as makani/train.py:87 "
                               "sets it (two-limb bf16 split, 3 products, ~4e-6; the reference's GPUs run TF32 there)" if spectral_train else
                               " in fp32-class arithmetic (three-limb bf16 split, 1.8e-7)")) if amp else "fp32",
                       "spectral_arithmetic": ops.gemm_mode(),
                       "multistep_count": args.multistep_count,
                       "multistep_checkpoint": bool(args.multistep_checkpoint),
                       "collectives": (dist.get_backend() if world > 1 else None),
                       "launch": ("hipGraph replay of the captured step" if graph is not None else "eager"),
                       "channel_gemm": "hip (csrc/conv1x1.hip)"},
            "peak_hbm_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2),
            "final_loss": final_loss,
        }
        if graph_note:
            out["note"] = graph_note
    if rank == 0 and args.full:
        prof = ops.PROFILER.summary()           # timed region: the dominant kernel (or everything with --warmup 0)
        # dominant HIP kernel = the kernel family with the largest accumulated time among our launches (what the
        # rocprofv3 --stats table of the same command shows on top); its numbers come from the timed steps
        if not (dom_family and any(m in prof for m in dom_members)):
            dom_family, dom_members = dominant_family(prof)
        kernels = kernel_table(warm_prof, prof, event_steps)
        pmc = load_pmc_traffic(fcn3) if (args.config in ("sfno_sc3_layers8_edim384", "fcn3_sc2_edim45_layers10") and msize == 1) else {}
        roofline = roofline_of(dom_family, dom_members, prof, ops.gemm_mode(), pmc.get(dom_family)) if dom_family else None
        # the runners-up, from the fully profiled warm-up step (one launch set, not an average over the timed steps)
        others = []
        if warm_prof:
            fams = {}
            for k in warm_prof:
                fams.setdefault(kernel_family(k), []).append(k)
            rank_f = sorted(fams, key=lambda f: -sum(warm_prof[k]["ms_total"] for k in fams[f]))
            for f in [f for f in rank_f if f != dom_family][:4]:
                others.append(roofline_of(f, sorted(fams[f]), warm_prof, ops.gemm_mode(), pmc.get(f)))
        hip_ms = sum(v["ms_per_step"] for v in kernels.values())
        out.update({"exact_fp32_spectral": exact, "roofline": roofline, "roofline_runners_up": others, "hip_kernels": kernels,
                    "hip_kernel_ms_per_step": round(hip_ms, 2)})
        if msize > 1:
            # what this rank (rank 0) puts on the links per step in the distributed transforms, by size of the process group the
            # all-to-all runs over (h, w or h x w) — to be read against SURVEY.md §8(e)'s 9.4 ms/step communication budget
            out["exchange_per_step_rank0"] = dict(comm_stats, total_MB_sent=round(sum(v["MB_sent"] for v in comm_stats.values()), 2),
                                                  schedule=("fused (one h x w all-to-all between FFT and Legendre transform)"
                                                            if os.environ.get("MAKANI_AMD_DIST_FUSED", "1") == "1" else "transpose by transpose"))
        if graph is not None and roofline:
            roofline["timing"] = (f"HIP events around the launches in {event_steps} eager steps run right after the timed region "
                                  "(the timed steps are hipGraph replays, whose nodes cannot carry events)")
        if world == 1 and not args.no_sht_metric and args.config == "sfno_sc3_layers8_edim384":
            del model, net, opt
            torch.cuda.empty_cache()
            print("[bench] train loop done; measuring fwd SHT", file=sys.stderr, flush=True)
            out["fwd_sht"] = sht_bandwidth(device)
            print("[bench] fwd SHT done; CPU baseline", file=sys.stderr, flush=True)
        # roofline.traffic measured in THIS run: the two counter passes are child runs of this script under rocprofv3.  They
        # finish BEFORE the CPU baseline starts (each builds the model on the host and precomputes the Legendre matrices in fp64:
        # beside the baseline they competed for its cores — ADVICE r5), at the price of about a minute of wall time
        pmc_thread, pmc_live = None, {}
        want_pmc = (world == 1 and not args.no_pmc and roofline is not None and args.multistep_count == 1
                    and args.config in ("sfno_sc3_layers8_edim384", "fcn3_sc2_edim45_layers10"))
        if want_pmc:
            # the counter passes build their own copy of the model: give the memory of this process back first (FourCastNet3
            # holds 128 GB per copy)
            model = net = opt = graph = graph_loss = loss = loss_fn = inp = tar = None      # noqa: F841 (drops the references)
            import gc as _gc
            _gc.collect()
            torch.cuda.empty_cache()
            import threading
            pmc_thread = threading.Thread(target=lambda: pmc_live.update(zip(("data", "note"), live_pmc_traffic(args.config, spectral=args.spectral))), daemon=True)
            pmc_thread.start()
            pmc_thread.join(timeout=900)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.config, parity=probe)
            out["parity_rel_l2"] = probe.finish() if probe is not None else None
        else:
            out["cpu_baseline"] = None
        if pmc_thread is not None:
            pmc_thread.join(timeout=900)
            live = pmc_live.get("data") or {}
            for r in [out.get("roofline")] + list(out.get("roofline_runners_up") or []):
                if not r:
                    continue
                if r["kernel"] in live:
                    r["traffic"] = live[r["kernel"]]
                    r["traffic_source"] = pmc_live.get("note")
                elif r.get("traffic") is not None:
                    r["traffic_source"] = (f"profiles/{PMC_TRAFFIC_FCN3 if fcn3 else PMC_TRAFFIC} (committed counter passes of the same "
                                           f"command; the live passes of this run gave nothing for this family: {pmc_live.get('note')})")
                else:
                    r["traffic_source"] = f"none: {pmc_live.get('note')}"
        elif out.get("roofline") and out["roofline"].get("traffic") is not None:
            out["roofline"]["traffic_source"] = f"profiles/{PMC_TRAFFIC_FCN3 if fcn3 else PMC_TRAFFIC} (committed counter passes of the same command)"
    if world > 1:
        dist.barrier()
        if capture_tried:
            # a captured step (replayed, or discarded because another rank's capture failed) holds RCCL's send / recv kernels:
            # tearing the communicator down after such a capture hangs (tools/probes/rccl_graph_probe.py) — the rank prints its
            # result and leaves without the teardown
            torch.cuda.synchronize()
            if out is not None:
                print(json.dumps(out), flush=True)
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        dist.destroy_process_group()
    return out


# --------------------------------------------------------------------------- #
# launcher: N ranks, one per GPU, headline + secondary measurement
# --------------------------------------------------------------------------- #
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_cmd(args, parallelism, dump=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--gpus", str(args.gpus), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--config", args.config, "--parallelism", parallelism, "--no-sht-metric",
           "--no-cpu-baseline", "--multistep-count", str(args.multistep_count), "--graph", args.graph, "--spectral", args.spectral]
    if args.full:
        cmd.append("--full")
    if dump and args.dump_outputs:
        cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
    if args.fp32:
        cmd.append("--fp32")
    if args.zero:
        cmd.append("--zero")
    if args.multistep_checkpoint:
        cmd.append("--multistep-checkpoint")
    return cmd


def _run_phase(args, parallelism, ranks, world, port, timeout_s, dump=False):
    """start one worker process per rank in ``ranks`` (all N when this script is the launcher, only our own when the
    driver's torch.distributed.run started one copy of this script per GPU), wait, return rank 0's JSON (or None) and
    an error string"""
    import subprocess
    procs = []
    for r in ranks:
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"),
                   MASTER_PORT=str(port))
        for k in [k for k in env if k.startswith("TORCHELASTIC_")]:
            del env[k]                     # the worker makes its own TCP store at MASTER_PORT (not the launcher agent's)
        env.setdefault("LOCAL_RANK", str(r))
        if len(ranks) > 1:
            env["LOCAL_RANK"] = str(r)
        if (os.environ.get("MAKANI_AMD_BENCH_BACKEND", "nccl") != "nccl" and world > 1 and torch.cuda.device_count() == 1
                and os.environ.get("MAKANI_AMD_BENCH_CU_MASK", "0") == "1"):
            # the functional mode "N ranks on ONE GPU over gloo", optionally with disjoint compute units per rank (isolates the
            # ranks' kernel timings; no longer needed for correct results: makani_amd/comm.py share_gpu); the variable must be
            # in the worker's environment before its HIP runtime starts
            per = max(1, 256 // world)
            env["HSA_CU_MASK"] = f"0:{r * per}-{(r + 1) * per - 1}"
        keep_out = (r == 0)
        procs.append((r, subprocess.Popen(_worker_cmd(args, parallelism, dump), env=env, stdout=subprocess.PIPE if keep_out else subprocess.DEVNULL,
                                          stderr=None, text=True)))
    result, err = None, None
    deadline = time.time() + timeout_s
    for r, pr in procs:
        try:
            so, _ = pr.communicate(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            pr.kill()                      # exactly the process we started
            so, _ = pr.communicate()
            err = f"rank {r}: no result within {timeout_s} s"
        if pr.returncode not in (0, None) and err is None:
            err = f"rank {r}: exit code {pr.returncode}"
        if r == 0 and so:
            lines = [l for l in so.splitlines() if l.startswith("{")]
            if lines:
                try:
                    result = json.loads(lines[-1])
                except ValueError:
                    pass
    return result, err


def launch(args):
    """N > 1.  Phase 1: the headline parallelism; phase 2 (--full only): plain data parallelism as ``secondary`` (skipped when
    the headline already is dp or with --no-secondary).  Each phase is its own set of worker processes with its own
    rendezvous port, so a failure in one (say, an RCCL all-to-all problem) cannot take the other measurement with it."""
    under_torchrun = int(os.environ.get("WORLD_SIZE", "1")) > 1
    world = int(os.environ["WORLD_SIZE"]) if under_torchrun else args.gpus
    rank = int(os.environ.get("RANK", "0")) if under_torchrun else 0
    ranks = [rank] if under_torchrun else list(range(world))
    base_port = int(os.environ.get("MASTER_PORT", "0")) if under_torchrun else 0
    head = args.parallelism if args.parallelism != "auto" else default_parallelism(world, args.config)
    phases = [head] + (["dp"] if (head != "dp" and args.full and not args.no_secondary) else [])
    timeout_s = int(os.environ.get("MAKANI_AMD_BENCH_PHASE_TIMEOUT", "360"))
    results, errors = {}, {}
    if under_torchrun:                         # the copies of this script agree on each phase's outcome over a host-side group
        import datetime
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=timeout_s + 300))
    nport = 0
    for par in phases:
        # the spatial split runs the fused exchange schedule (makani_amd/dist_pipeline.py); should that phase fail — its RCCL
        # branches with more than one rank cannot be exercised in the development environment — it is repeated once with the
        # transpose-by-transpose schedule before the data-parallel measurement is reported instead
        # ... and before that once with eager launches instead of the captured step (hipGraph capture of RCCL collectives has
        # only ever run with ONE rank here: tests/test_gpu_distributed.py::test_hipgraph_capture_of_the_distributed_blocks_with_rccl_world1)
        gloo = os.environ.get("MAKANI_AMD_BENCH_BACKEND", "nccl") != "nccl"
        eager = [] if (gloo or args.graph == "off") else [dict(MAKANI_AMD_BENCH_GRAPH="off")]
        attempts = [dict()] + eager + ([] if par == "dp" else [dict(MAKANI_AMD_BENCH_GRAPH="off", MAKANI_AMD_DIST_FUSED="0")])
        for env_over in attempts:
            fused = env_over.get("MAKANI_AMD_DIST_FUSED")
            nport += 1
            port = (base_port + nport) if under_torchrun else _free_port()
            os.environ.update(env_over)
            # the first attempt (captured step) gets a shorter leash: a capture that hangs must not eat the time of the eager retry
            first_graph = (not env_over) and eager
            res, err = _run_phase(args, par, ranks, world, port, min(timeout_s, 200) if first_graph else timeout_s, dump=par == head)
            for k in env_over:
                os.environ.pop(k, None)
            if env_over and res is not None and not err:
                res["note"] = ("the first attempt of this phase failed; this line ran with " + ", ".join(f"{k}={v}" for k, v in env_over.items())
                               + " (eager launches instead of the captured step" + ("; transpose-by-transpose exchange schedule)" if fused else ")"))
            results[par], errors[par] = res, err
            ok = err is None and (rank != 0 or res is not None)
            if under_torchrun:                 # every rank's copy of this script must take the same decision about a retry
                flag = torch.tensor([1 if ok else 0])
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = bool(flag.item())
                if not ok and errors[par] is None:
                    errors[par] = "another rank's worker failed"
            if rank == 0:
                tag = par + (" (" + ", ".join(f"{k}={v}" for k, v in env_over.items()) + ")" if env_over else "")
                print(f"[bench] phase {tag}: {'ok' if ok else 'FAILED: ' + str(errors[par])}", file=sys.stderr, flush=True)
            if ok:
                break
    if under_torchrun:
        dist.destroy_process_group()
    if rank != 0:
        return None
    out = results.get(head) if not errors.get(head) else None
    sec = results.get("dp") if (len(phases) > 1 and not errors.get("dp")) else None
    if out is None and sec is not None:          # the headline split did not run: report data parallelism, and say so
        out, sec = sec, None
        out["note"] = f"headline parallelism {head} failed ({errors.get(head)}); this line is the data-parallel measurement"
    if out is None:
        raise SystemExit(f"bench: no phase produced a result: {errors}")
    if sec is not None:
        out["secondary"] = {k: sec[k] for k in ("value", "unit", "ms_per_step", "scaling", "steps", "warmup", "final_loss")}
        out["secondary"]["parallelism"] = sec["config"]["parallelism"]
        out["secondary"]["global_batch"] = sec["config"]["global_batch"]
    out["cpu_baseline"] = None                   # rank 0 at N = 1 only
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="sfno_sc3_layers8_edim384", choices=list(CONFIGS),
                    help="sfno_sc3_layers8_edim384 = BASELINE configs[1] (the headline; with --multistep-count 4: configs[4]); "
                         "fcn3_sc2_edim45_layers10 = configs[3] (FourCastNet3, ensemble CRPS recipe); *_debug = small stand-ins")
    ap.add_argument("--fp32", action="store_true", help="disable bf16 autocast (not the BASELINE metric)")
    ap.add_argument("--spectral", default="train", choices=["train", "exact"],
                    help="fp32 matrix products of the spectral path: 'train' (default) = torch.backends.cuda.matmul.allow_tf32 = True, "
                         "as the reference's training entry point sets it (makani/train.py:87-88): two-limb bf16 split; 'exact' = torch's "
                         "default: three-limb split, fp32 round-off class")
    ap.add_argument("--no-exact", action="store_true", help="skip the secondary measurement of the step with --spectral exact arithmetic")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sht-metric", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="do not collect roofline.traffic with rocprofv3 counter passes in this run "
                                                          "(the committed profiles/ file is used instead)")
    ap.add_argument("--parallelism", default=os.environ.get("MAKANI_AMD_PARALLELISM", "auto"),
                    help="'auto' (default: dp on one or two GPUs; on 4 / 8 GPUs the north-star split h x w over all N GPUs — "
                         "4: h4w1, 8: h4w2 — strong scaling), 'dp' (one sample per GPU, weak scaling) or 'hHwW': spatial "
                         "model parallelism over H x W GPUs per model instance, remaining ranks data parallel")
    ap.add_argument("--no-secondary", action="store_true", help="N > 1: skip the second (data-parallel) measurement")
    ap.add_argument("--zero", action="store_true",
                    help="data parallelism with ZeRO-1: reduce-scatter the large gradients, shard the AdamW state over the data "
                         "group, all-gather the parameters (gloo-tested; off by default because RCCL with N > 1 ranks cannot "
                         "be exercised in the development environment)")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="capture the train step in a hipGraph and replay it (auto: on one GPU)")
    ap.add_argument("--multistep-count", type=int, default=1,
                    help="autoregressive rollout length per sample (makani's --multistep_count, BASELINE configs[4]); "
                         "1 = the headline single-step metric")
    ap.add_argument("--multistep-checkpoint", action="store_true",
                    help="recompute each rollout step's network call in backward (makani's --multistep_checkpoint)")
    ap.add_argument("--full", action="store_true",
                    help="also take every measurement beside the headline: per-kernel table and roofline (with live counter "
                         "passes), the step with exact fp32 spectral arithmetic, forward SHT bandwidth, CPU baseline and in-run "
                         "parity against the oracle; N > 1: exchange volume and the data-parallel secondary phase")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (loss, gradients and updated "
                         "parameters; large tensors as a fixed seeded sample) as DIR/<name>.npy")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-mode", default="fwd", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-state", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_worker and CONFIGS.get(args.cpu_worker, {}).get("kind") == "fcn3":
        _cpu_worker_fcn3(args.cpu_worker, args.cpu_state, args.cpu_out)
        return
    if args.cpu_worker:
        _cpu_worker(args.cpu_worker, args.cpu_mode, args.cpu_state, args.cpu_out)
        return
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.worker or (args.gpus <= 1 and env_world <= 1):
        out = run_worker(args)                   # a rank of a launched job, or the plain one-GPU run (in process)
    else:
        out = launch(args)
    if out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
