"""The cosine of the solar zenith angle — the ``add_zenith`` input channel — computed on the device (``csrc/zenith.hip``).

``cos_zenith_angle(time, lon, lat)`` takes the arguments of ``makani/third_party/climt/zenith_angle_v2.py`` and returns the
``(T, H, W)`` planes as a GPU tensor.  ``ZenithFeatures`` is the per-step form: it holds the grid and a device buffer of valid
times ``(B, n_history + 1)`` and returns the ``(B, n_history + 1, H, W)`` tensor that ``Preprocessor2D`` and the stepper
wrappers take as unpredicted features (``model_package.py:251-296``); ``advance()`` moves the times on by ``dt_hours`` on the
device, so ``forward(); advance()`` can be captured in a hipGraph and every replay gives the planes of the next valid time.

What differs from the reference:

* the time scalars (Julian centuries, obliquity, ecliptic longitude, declination, right ascension, GMST) are evaluated in fp64
  from int64 microseconds; the reference holds the days since J2000 and the sidereal-time polynomial in fp32 and is up to
  2.0e-3 away from the fp64 value of its own formulas.  The field itself is formed in fp32 as there.
* the grid is rank 1 x rank 1: ``lat (H)`` and ``lon (W)`` in degrees.  The reference's 2-D ``np.meshgrid(lon, lat)`` pair is
  accepted when it is such an outer product and raises ``ValueError`` otherwise.
* under an h x w split a rank passes (``from_params``: takes from ``comm``) its own slices of ``lat`` / ``lon``; its planes
  are bit for bit the slices of the serial planes.
* nothing runs on the CPU: a CPU tensor raises, and datetimes are converted on the host once, when they are handed in.
"""
import datetime as _dt

import numpy as np
import torch
import torch.nn as nn

from . import _lib

_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)


def _times_us(time):
    """host datetimes (``datetime`` — naive ones are UTC —, ``numpy.datetime64``, or sequences / arrays of them) as a flat
    int64 array of UTC microseconds since the Unix epoch"""
    arr = np.atleast_1d(np.asarray(time)).reshape(-1)
    if np.issubdtype(arr.dtype, np.datetime64):
        return arr.astype("datetime64[us]").astype(np.int64)
    out = np.empty(arr.shape, dtype=np.int64)
    for i, t in enumerate(arr):
        if isinstance(t, np.datetime64):
            out[i] = t.astype("datetime64[us]").astype(np.int64)
        elif isinstance(t, _dt.datetime):
            aware = t.replace(tzinfo=_dt.timezone.utc) if t.tzinfo is None else t
            out[i] = (aware - _EPOCH) // _dt.timedelta(microseconds=1)
        else:
            raise TypeError(f"time entries have to be datetime.datetime or numpy.datetime64, got {type(t).__name__}")
    return out


def _device_times(time, device):
    """``time`` as a flat device int64 tensor: a GPU int64 tensor is used as it is, host datetimes are converted and uploaded"""
    if isinstance(time, torch.Tensor):
        _lib.need_gpu(time, "zenith features")
        if time.dtype != torch.int64:
            raise TypeError(f"a time tensor holds int64 UTC microseconds since the Unix epoch, got {time.dtype}")
        return time.reshape(-1)
    return torch.from_numpy(_times_us(time)).to(device)


def grid_vectors(lon, lat):
    """``(lat (H), lon (W))`` as fp64 numpy vectors in degrees, from 1-D vectors or from the reference's 2-D pair
    ``lon_grid, lat_grid = np.meshgrid(lon, lat)``, which has to be that outer product exactly"""
    def host(v):
        if isinstance(v, torch.Tensor):
            _lib.need_gpu(v, "zenith features")
            v = v.detach().cpu().numpy()
        return np.asarray(v, dtype=np.float64)
    lon, lat = host(lon), host(lat)
    if lon.ndim == 2 and lat.ndim == 2:
        if lon.shape != lat.shape:
            raise ValueError(f"lon grid {lon.shape} and lat grid {lat.shape} differ in shape")
        if not (np.array_equal(lon, np.broadcast_to(lon[:1], lon.shape)) and np.array_equal(lat, np.broadcast_to(lat[:, :1], lat.shape))):
            raise ValueError("the 2-D lon / lat grids are not the meshgrid of a longitude and a latitude vector: the zenith "
                             "kernel takes a rank-1 x rank-1 grid (lon constant along H, lat constant along W)")
        lon, lat = lon[0], lat[:, 0]
    if lon.ndim != 1 or lat.ndim != 1:
        raise ValueError(f"lon / lat are 1-D vectors or a 2-D meshgrid pair, got {lon.ndim}-D and {lat.ndim}-D")
    return np.ascontiguousarray(lat), np.ascontiguousarray(lon)


def zenith_tables(lat_deg, lon_deg):
    """the kernel's fp32 tables ``sin lat (H) | cos lat (H) | cos lon (W) | sin lon (W)`` of fp64 device vectors in degrees"""
    _lib.need_gpu(lat_deg, "zenith features")
    for v in (lat_deg, lon_deg):
        if v.dtype != torch.float64 or v.dim() != 1 or not v.is_contiguous() or v.device != lat_deg.device:
            raise TypeError(f"the grid vectors are contiguous 1-D float64 tensors on one GPU, got {v.dtype} {tuple(v.shape)} on {v.device} "
                            f"(a module cast with .float() / .bfloat16() loses them: pass dtype= to ZenithFeatures instead)")
    H, W = lat_deg.numel(), lon_deg.numel()
    tab = torch.empty(2 * (H + W), dtype=torch.float32, device=lat_deg.device)
    with torch.cuda.device(lat_deg.device):
        _lib.check(_lib.lib().mk_zenith_tables(_lib.ptr(lat_deg), _lib.ptr(lon_deg), _lib.ptr(tab), H, W, _lib.stream()), "mk_zenith_tables")
    return tab


def cos_zenith_planes(times, tab, out):
    """Write plane ``(b, t)`` of the times ``times (Bt, T)`` (device int64; ``Bt = 1`` is shared by the batch) into
    ``out[b, t]``.  ``out (B, T, H, W)`` f32 | bf16 may be a view into a larger tensor (channel slots of a feature buffer): its
    planes have to be contiguous, the batch and level strides are free.  One launch; returns ``out``."""
    _lib.need_gpu(out, "zenith features")
    B, T, H, W = out.shape
    if tuple(times.shape) not in ((B, T), (1, T)) or times.dtype != torch.int64 or not times.is_contiguous():
        raise ValueError(f"times {tuple(times.shape)} {times.dtype} do not fit planes {tuple(out.shape)}: need contiguous int64 (B | 1, T)")
    if tab.numel() != 2 * (H + W) or tab.dtype != torch.float32 or not tab.is_contiguous():
        raise ValueError(f"tables of {tab.numel()} {tab.dtype} entries do not belong to a {H} x {W} grid")
    if not (times.device == tab.device == out.device):
        raise ValueError(f"times ({times.device}), tables ({tab.device}) and out ({out.device}) live on different devices")
    if out.stride(3) != 1 or out.stride(2) != W or out.stride(0) < 0 or out.stride(1) < 0:
        raise ValueError(f"the planes of out have to be contiguous (strides {out.stride()})")
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().mk_cos_zenith(_lib.ptr(times), times.shape[0], _lib.ptr(tab), _lib.ptr(out), _lib.dtype_code(out), B, T,
                                            H, W, out.stride(0), out.stride(1), _lib.stream()), "mk_cos_zenith")
    return out


def cos_zenith_angle(time, lon, lat, out=None, dtype=torch.float32, device=None):
    """``cos_zenith_angle(time, lon, lat)`` of the reference on the device: ``(T, H, W)`` planes of ``dtype`` (f32 | bf16) at
    the UTC times ``time`` — a GPU int64 tensor of microseconds since the Unix epoch, or host datetimes /
    ``numpy.datetime64`` — on the grid ``lon`` / ``lat`` in degrees (1-D, or the 2-D meshgrid pair).  ``out``: write there
    instead (planes contiguous, level stride free).  The device is that of ``out``, of a tensor argument, or the current one."""
    for a in (out, time, lon, lat):
        if isinstance(a, torch.Tensor):
            _lib.need_gpu(a, "zenith features")
            device = a.device if device is None else device
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lat_v, lon_v = grid_vectors(lon, lat)
    times = _device_times(time, device).contiguous()
    T, H, W = times.numel(), lat_v.size, lon_v.size
    if out is None:
        out = torch.empty(T, H, W, dtype=dtype, device=device)
    elif tuple(out.shape) != (T, H, W):
        raise ValueError(f"out has shape {tuple(out.shape)}, the planes {(T, H, W)}")
    tab = zenith_tables(torch.from_numpy(lat_v).to(device), torch.from_numpy(lon_v).to(device))
    cos_zenith_planes(times.view(1, T), tab, out.unsqueeze(0))
    return out


class ZenithFeatures(nn.Module):
    """The zenith planes of a model's input window as unpredicted features, ``(B, n_history + 1, H, W)``.

    ``lat (H)`` / ``lon (W)``: this rank's grid vectors in degrees.  ``dt_hours``: what ``advance()`` adds.  ``dhours_history``:
    spacing of the history levels; when given, ``set_time`` also takes ONE time per member (or one for all) and expands it to the
    window ``t - (n_history - k) dhours_history``.  Buffers (non-persistent): ``lat_deg``, ``lon_deg`` fp64, ``times``
    ``(B | 1, n_history + 1)`` int64 microseconds.  ``set_time`` re-uses the ``times`` storage while its shape stays, so a
    captured ``forward(); advance()`` keeps reading the buffer ``set_time`` writes."""

    def __init__(self, lat, lon, n_history=0, dt_hours=6, dhours_history=None, dtype=torch.float32):
        super().__init__()
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"unsupported dtype {dtype} (float32 / bfloat16 only)")
        lat_v, lon_v = (np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1) for v in (lat, lon))
        self.n_history, self.dtype = int(n_history), dtype
        self.dt_us = round(float(dt_hours) * 3.6e9)
        self.dhist_us = None if dhours_history is None else round(float(dhours_history) * 3.6e9)
        self.register_buffer("lat_deg", torch.from_numpy(lat_v.copy()), persistent=False)
        self.register_buffer("lon_deg", torch.from_numpy(lon_v.copy()), persistent=False)
        self.register_buffer("times", torch.zeros(1, self.n_history + 1, dtype=torch.int64), persistent=False)
        self._tab = None

    @classmethod
    def from_params(cls, params, dtype=torch.float32):
        """From the reference's parameters: ``lat`` / ``lon`` (degrees; absent: the equiangular grid of ``model_package.py:155-164``
        at ``img_shape_x/y``), ``n_history``, and ``dt * dhours`` hours per step and per history level.  Under a spatial split
        (``comm.get_size("h") / ("w") > 1``) the module holds this rank's slices of the vectors."""
        from . import comm
        from .distributed import compute_split_shapes
        get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
        lat, lon = get("lat", None), get("lon", None)
        lat = np.linspace(90.0, -90.0, get("img_shape_x"), endpoint=True) if lat is None else np.asarray(lat, dtype=np.float64)
        lon = np.linspace(0.0, 360.0, get("img_shape_y"), endpoint=False) if lon is None else np.asarray(lon, dtype=np.float64)
        for name, n in (("h", comm.get_size("h")), ("w", comm.get_size("w"))):
            if n > 1:
                v = lat if name == "h" else lon
                shapes, r = compute_split_shapes(v.size, n), comm.get_rank(name)
                v = v[sum(shapes[:r]):sum(shapes[:r + 1])]
                lat, lon = (v, lon) if name == "h" else (lat, v)
        hours = (get("dt", 1) or 1) * (get("dhours", 1) or 1)
        return cls(lat, lon, n_history=get("n_history", 0) or 0, dt_hours=hours, dhours_history=hours, dtype=dtype)

    def extra_repr(self):
        return f"grid=({self.lat_deg.numel()}, {self.lon_deg.numel()}), n_history={self.n_history}, dt_us={self.dt_us}"

    def set_time(self, time, batch_size=1):
        """Valid times of the window (``model_package.py:281-294``): ``batch_size * (n_history + 1)`` of them, one per member and
        history level, member-major; or ``n_history + 1``, one window shared by every member.  Anything else raises the
        reference's ``ValueError`` (but see ``dhours_history``).  A GPU int64 tensor is copied on the device."""
        nhist = self.n_history + 1
        _lib.need_gpu(self.times, "zenith features")
        t = _device_times(time, self.times.device)
        n = t.numel()
        if n not in (batch_size * nhist, nhist):
            if self.dhist_us is None or n not in (batch_size, 1):
                raise ValueError(f"add_zenith: got {n} time(s) for a batch of {batch_size} with n_history={nhist - 1}. Pass either "
                                 f"{batch_size * nhist} times (one per member per history step, member-major) or {nhist} time(s) "
                                 f"to share one history window across the whole batch.")
            back = torch.arange(-self.n_history, 1, dtype=torch.int64, device=t.device) * self.dhist_us
            t = t.view(n, 1) + back
        t = t.reshape(-1, nhist)
        if tuple(t.shape) == tuple(self.times.shape):
            self.times.copy_(t)
        else:
            self.register_buffer("times", t.clone(), persistent=False)
        return self

    def tables(self):
        if self._tab is None or self._tab.device != self.lat_deg.device:
            self._tab = zenith_tables(self.lat_deg, self.lon_deg)
        return self._tab

    def forward(self, batch_size, out=None):
        """the planes at the current times, ``(batch_size, n_history + 1, H, W)``; ``out``: a view to write them into"""
        _lib.need_gpu(self.times, "zenith features")
        if self.times.shape[0] not in (1, batch_size):
            raise ValueError(f"the times were set for a batch of {self.times.shape[0]}, not {batch_size}")
        if out is None:
            out = torch.empty(batch_size, self.n_history + 1, self.lat_deg.numel(), self.lon_deg.numel(), dtype=self.dtype,
                              device=self.times.device)
        elif tuple(out.shape) != (batch_size, self.n_history + 1, self.lat_deg.numel(), self.lon_deg.numel()):
            raise ValueError(f"out has shape {tuple(out.shape)}")
        return cos_zenith_planes(self.times, self.tables(), out)

    def advance(self, steps=1):
        """``times += steps * dt_hours`` on the device, stream-ordered behind ``forward``"""
        _lib.need_gpu(self.times, "zenith features")
        with torch.cuda.device(self.times.device):
            _lib.check(_lib.lib().mk_zenith_advance(_lib.ptr(self.times), self.times.numel(), int(steps) * self.dt_us, _lib.stream()),
                       "mk_zenith_advance")
        return self
