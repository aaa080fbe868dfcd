"""The zenith restatement against the reference's own output, and the host side of makani_amd/zenith.py, without a GPU."""
import datetime as dt
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _zenith_ref as ref          # noqa: E402

# 1.25 x the measured fp32-arithmetic error of the reference, 2.026e-3 (tools/make_zenith_golden.py)
D_REF = 2.6e-3


def test_restatement_states_the_formulas_of_the_reference():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zenith.npz"))
    assert np.array_equal(g["times_us"], ref.times_us())
    err = np.abs(ref.cos_zenith(g["times_us"], g["lat"], g["lon"]) - g["cosz"]).max(axis=(1, 2))
    print("max |fp64 restatement - reference| per time:", err)
    assert err.max() <= D_REF and err[1] <= 2e-6          # at jc = 0 the reference's fp32 time arithmetic is exact


def test_host_side_times_and_grids():
    from makani_amd import zenith
    stamps = [dt.datetime(1979, 1, 1), dt.datetime(2000, 1, 1, 12, tzinfo=dt.timezone.utc), np.datetime64("2024-02-29T18:00"),
              dt.datetime(2050, 1, 1, 0, 59, 59, 500000, tzinfo=dt.timezone(dt.timedelta(hours=1)))]
    assert np.array_equal(zenith._times_us(stamps), ref.times_us())
    lon_grid, lat_grid = np.meshgrid(np.linspace(0, 360, 8, endpoint=False), np.linspace(90, -90, 5))
    lat_grid[2, 3] += 1e-9
    with pytest.raises(ValueError, match="meshgrid"):
        zenith.grid_vectors(lon_grid, lat_grid)
