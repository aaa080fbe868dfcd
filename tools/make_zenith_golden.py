"""Record tests/golden/zenith.npz: the reference's own, unmodified ``cos_zenith_angle``
(makani/third_party/climt/zenith_angle_v2.py, fp32 arithmetic), imported through oracle.ref_shims, on a 13 x 24 equiangular grid
(poles included) at the four times of tests/_zenith_ref.py, with the times (int64 microseconds) and the grid vectors as data.
Prints d_ref, the largest distance between that output and the fp64 restatement tests/_zenith_ref.py: the error of the
reference's fp32 time arithmetic.  Needs the reference checkout (MAKANI_REFERENCE_ROOT); run from the repository
root:  python tools/make_zenith_golden.py"""
import datetime as dt
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    from oracle import ref_shims
    import _zenith_ref as R
    mod = ref_shims.import_reference_module("makani.third_party.climt.zenith_angle_v2")
    t_us = R.times_us()
    epoch = dt.datetime(1970, 1, 1, tzinfo=dt.timezone.utc)
    stamps = np.array([epoch + dt.timedelta(microseconds=int(t)) for t in t_us])
    lat, lon = np.linspace(90.0, -90.0, 13), np.linspace(0.0, 360.0, 24, endpoint=False)
    lon_grid, lat_grid = np.meshgrid(lon, lat)
    cosz = mod.cos_zenith_angle(stamps, lon_grid, lat_grid)
    assert cosz.dtype == np.float32 and cosz.shape == (4, 13, 24)
    want = R.cos_zenith(t_us, lat, lon)
    for s, c, w in zip(R.TIMES, cosz, want):
        print(f"{s:24s} max |reference - fp64 restatement| = {np.abs(c - w).max():.3e}")
    print(f"d_ref = {np.abs(cosz - want).max():.3e}")
    path = os.path.join(ROOT, "tests", "golden", "zenith.npz")
    np.savez_compressed(path, times_us=t_us, lat=lat, lon=lon, cosz=cosz)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
