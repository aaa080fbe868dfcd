"""fp64 restatement of ``MetricsHandler`` (makani/utils/metric.py): the whole update / reduce / finalize sequence, written from
its definition on top of the plane sums of tests/_metrics_ref.py.

Per ``update(prediction (B, [E,] C, H, W), target (B, C, H, W), loss, idt, weight)`` and per handle with channel list ch:
    t = target[:, ch];  if mask_target_nan and t holds a NaN anywhere:  m = [t is a number],  t <- where(m, t, 0),  w <- (w or 1) m
    value (per channel, summed over the batch b), with Q the normalised quadrature under w and x the member mean:
        L1     sum_b Q[|x - t|]                          RMSE   sqrt(sum_b Q[(x - t)^2]) scale
        ACC    sum_b Q[x't'] / (sqrt(Q[x'^2] Q[t'^2]) + 1e-8),  x' = x - climatology, t' = t - climatology
        CRPS   sum_b Q[fair crps] scale                  Spread sum_b sqrt(Q[sum_e (f_e - x)^2] / (E - 1)) scale
        SSR    sum_b sqrt(s / max(Q[(x - t)^2] - s / E, 1e-6)),  s = Q[sum_e (f_e - x)^2] / (E - 1)
        Rank Histogram  sum_b Q[[r = k]], k = 0 .. E
    counts = B if w is None else sum_b Q[w]              (one number per channel; a trailing unit axis for the histogram)
    curve[idt] <- curve[idt] + value  (RMSE: sqrt(curve[idt]^2 + value^2)),   counter[idt] <- counter[idt] + counts
``reduce`` combines the curves of the ranks of a "batch" group in the same way; ``finalize`` divides by the counter (RMSE: by its
square root), integrates ACC over the lead time (Simpson's rule on an even number of intervals, the trapezoid rule otherwise,
interval width 1 / steps) and assembles the scalar log entries.  Test helper: plain torch, shares no code with the kernels."""
import json
import math

import torch

import _crps_ref
import _metrics_ref as ref

ORDER = [("L1", "l1_var_names"), ("RMSE", "rmse_var_names"), ("ACC", "acc_var_names"), ("CRPS", "crps_var_names"),
         ("Spread", "spread_var_names"), ("SSR", "ssr_var_names"), ("Rank Histogram", "rh_var_names")]
DEFAULT_VARS = ["u10m", "t2m", "sp", "sst", "u500", "z500", "q500", "q50"]
SCALED = ("RMSE", "CRPS", "Spread")
ENSEMBLE = ("CRPS", "Spread", "SSR", "Rank Histogram")


def wb2_weights(img_shape):
    """weatherbench2's latitude weights, normalised to sum 1: the cosine differences of the cell bounds"""
    H, W = img_shape
    lats = torch.linspace(0, math.pi, H, dtype=torch.float64)
    bounds = torch.cat([torch.zeros(1, dtype=torch.float64), (lats[:-1] + lats[1:]) / 2, torch.full((1,), math.pi, dtype=torch.float64)])
    jac = torch.cos(bounds[:-1]) - torch.cos(bounds[1:])
    return ((2 * math.pi / W) * jac / (4 * math.pi)).unsqueeze(1).expand(H, W)


def time_weights(steps):
    n, width = steps - 1, 1.0 / steps
    if n % 2 == 0:
        w = [0.0] * (n + 1)
        for j in range(1, n // 2 + 1):
            w[2 * j - 2] += 1.0
            w[2 * j - 1] += 4.0
            w[2 * j] += 1.0
        return torch.tensor(w, dtype=torch.float64) * (width / 3.0)
    w = [width] * (n + 1)
    w[0] *= 0.5
    w[-1] *= 0.5
    return torch.tensor(w, dtype=torch.float64)


class Handler:
    def __init__(self, channel_names, img_shape, steps, dtxdh, lists, ensemble_size=1, climatology=None, scale=None, wb2=False,
                 mask_target_nan=True, quad_weight=None):
        """``lists``: {"l1_var_names": [...], ...} (missing keys: the reference's eight default variables; names absent from
        ``channel_names`` are dropped); ``quad_weight``: (H, W) fp64 weights of this rank's planes (default: the whole sphere)"""
        self.names, self.steps, self.dtxdh, self.mask = list(channel_names), steps, dtxdh, mask_target_nan
        self.E = ensemble_size
        self.q = quad_weight if quad_weight is not None else (wb2_weights(img_shape) if wb2 else ref.quadrature_weights(img_shape, normalize=True))
        self.clim = climatology.double() if climatology is not None else None
        self.scale = (scale.double().reshape(-1) if scale is not None else torch.ones(len(self.names), dtype=torch.float64))
        self.handles = []          # (name, channel names, channel indices)
        for name, key in ORDER:
            ch = [c for c in lists.get(key, [] if key == "rh_var_names" else DEFAULT_VARS) if c in self.names]
            if ch:
                self.handles.append((name, ch, [self.names.index(c) for c in ch]))
        self.curve = {n: torch.zeros((steps, len(ch)) + ((ensemble_size + 1,) if n == "Rank Histogram" else ()), dtype=torch.float64)
                      for n, ch, _ in self.handles}
        self.counter = {n: torch.zeros((steps, len(ch)) + ((1,) if n == "Rank Histogram" else ()), dtype=torch.float64)
                        for n, ch, _ in self.handles}
        self.valid = torch.zeros(2, dtype=torch.float64)          # loss, steps

    def value(self, name, idx, f, t, w):
        """f (B, E, n, H, W), t (B, n, H, W), w | None -> the batch-summed value of the handle, and its counts"""
        E = f.shape[1]
        x = sum(f[:, e] for e in range(E)) / E
        sc = self.scale[idx]
        if name in ("L1", "RMSE", "ACC"):
            bias = self.clim[0, idx] if (name == "ACC" and self.clim is not None) else None
            s = ref.det_sums(x, t, self.q, w, bias)
            if name == "L1":
                return s[..., 0].sum(0)
            if name == "RMSE":
                return s[..., 1].sum(0).sqrt() * sc
            return (s[..., 2] / ((s[..., 3] * s[..., 4]).sqrt() + 1e-8)).sum(0)
        if name == "CRPS":
            return _crps_ref.crps(f, t, self.q, w, "skillspread").sum(0) * sc
        skill, ss, hist = ref.ens_sums(f, t, self.q, w)
        if name == "Rank Histogram":
            return hist.sum(0)
        var = ss / torch.tensor(float(E - 1), dtype=torch.float64)
        if name == "Spread":
            return var.sqrt().sum(0) * sc
        return (var / torch.clamp(skill - var / E, min=1e-6)).sqrt().sum(0)

    def update(self, prediction, target, loss, idt, weight=None):
        f = prediction.double() if prediction.dim() == 5 else prediction.double().unsqueeze(1)
        tar = target.double()
        B = tar.shape[0]
        for name, _, idx in self.handles:
            t, w = tar[:, idx], (weight.double().expand(tar.shape)[:, idx] if weight is not None else None)
            if self.mask and bool(torch.isnan(t).any()):
                m = (~torch.isnan(t)).double()
                t = torch.where(m > 0, t, torch.zeros_like(t))
                w = m if w is None else w * m
            val = self.value(name, idx, f[:, :, idx], t, w)
            cnt = (torch.full((len(idx),), float(B), dtype=torch.float64) if w is None
                   else (self.q.double() * w).sum(dim=(-2, -1)).sum(0))
            if name == "Rank Histogram":
                cnt = cnt.unsqueeze(-1)
            self.curve[name][idt] = (self.curve[name][idt] ** 2 + val ** 2).sqrt() if name == "RMSE" else self.curve[name][idt] + val
            self.counter[name][idt] = self.counter[name][idt] + cnt
        if idt == 0:
            self.valid += torch.tensor([float(loss), 1.0], dtype=torch.float64)

    def reduce(self, others):
        """combine with the handlers of the other ranks of the "batch" group"""
        for name, _, _ in self.handles:
            vals = torch.stack([h.curve[name] for h in [self] + list(others)])
            self.curve[name] = (vals ** 2).sum(0).sqrt() if name == "RMSE" else vals.sum(0)
            self.counter[name] = torch.stack([h.counter[name] for h in [self] + list(others)]).sum(0)
        self.valid = self.valid + sum(h.valid for h in others)

    def finalize(self):
        """-> (final {name: curve}, integral {name: (channels,)}, logs {"base": .., "metrics": ..} without the table)"""
        final, integral = {}, {}
        for name, _, _ in self.handles:
            c = self.counter[name]
            final[name] = self.curve[name] / (c.sqrt() if name == "RMSE" else c)
        if "ACC" in final:
            integral["ACC"] = (final["ACC"] * time_weights(self.steps).unsqueeze(1)).sum(0)
        logs = {"base": {"validation steps": self.valid[1].item(), "validation loss": (self.valid[0] / self.valid[1]).item()}, "metrics": {}}
        for name, ch, _ in self.handles:
            if name == "Rank Histogram":
                continue
            rows = ([0] if name != "ACC" else []) + [self.steps - 1]
            for index in rows:
                for i, var in enumerate(ch):
                    logs["metrics"][f"validation {name} {var}({(index + 1) * self.dtxdh})"] = final[name][index, i].item()
                if name == "ACC":
                    for i, var in enumerate(ch):
                        logs["metrics"][f"validation {name} AUC {var}({self.steps * self.dtxdh})"] = integral["ACC"][i].item()
        return final, integral, logs


# ---- the recorded cases (tools/make_metricshandler_golden.py) ------------------------------------------------------------
def case_names(golden):
    return [k[:-5] for k in golden.files if k.endswith("/meta")]


def case_meta(golden, name):
    return json.loads(str(golden[f"{name}/meta"]))


def case_handler(golden, name):
    meta = case_meta(golden, name)
    kw = meta["handler_kwargs"]
    clim = torch.from_numpy(golden[f"{name}/clim"].astype("float64")) * 2.0 ** -meta["shift"] if meta["climatology"] else None
    return Handler(meta["channel_names"], (meta["img_shape_x_resampled"], meta["img_shape_y_resampled"]), meta["steps"], meta["dtxdh"],
                   {k: v for k, v in kw.items() if k.endswith("_var_names")}, ensemble_size=meta["E"], climatology=clim,
                   scale=torch.from_numpy(golden["scale"]), wb2=kw.get("wb2_compatible", False))


def case_call(golden, name, call):
    """(prediction, target, loss, idt, weight | None) of a recorded call, fp32"""
    meta = case_meta(golden, name)
    get = lambda k, s: torch.from_numpy(golden[f"{name}/call{call}/{k}"].astype("float32")) * 2.0 ** -s          # noqa: E731
    prd, tar = get("prd", meta["shift"]), get("tar", meta["shift"])
    if meta["E"] == 1:
        prd = prd[:, 0]
    wgt = get("wgt", meta["wshift"]) if meta["weights"] else None
    if f"{name}/call{call}/nan" in golden.files:
        tar = torch.where(torch.from_numpy(golden[f"{name}/call{call}/nan"]) > 0, torch.full_like(tar, float("nan")), tar)
    return prd, tar, 0.25 * (call + 1), call % meta["steps"], wgt
